"""Guard bands for include/kvzip_hip_branch.h and ForkedCache.commit: the calls run on buffers carved from a guarded arena
(tests/guards.py) - exactly as large as declared, 256-byte aligned, hashed surroundings.  The kernels here only move bytes, so the
buffers keep the arena's position-dependent pattern as their content: kvz_fork_branch_copy may write dst[0:rows] of every layer and
head and nothing else (rows >= rows_i, sources, bystanders and guards still hold the pattern afterwards), and commit may write the
declared slack rows of the base cache - rows len_h + off .. + t of every head - and nothing else."""
import ctypes as C
import types

import pytest
import torch

from guards import Arena, frozen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("Hkv,D", [(3, 128), (1, 64)])
def test_branch_copy_writes_only_the_destination_rows(Hkv, D, dtype):
    from kvzip_amd import ops
    lib = ops._lib.load()
    B, caps = 5, (8, 40, 40)
    for layers, pairs, rows in (((0, 1, 2), [(2, 0), (2, 4), (2, 1)], [7, 1, 0]), ((0, 1, 2), [(4, 1), (0, 3)], [8, 7]),
                                ((1, 2), [(2, 0), (2, 4), (2, 1)], [33, 33, 7]), ((1, 2), [(4, 1), (0, 3)], [1, 40]), ((0, 1, 2), [], [])):
        a = Arena(DEV)
        tk, tv = [], []
        for l in layers:
            for name, lst in (("k", tk), ("v", tv)):
                t = a.carve(f"tail_{name}{l}", ((B, Hkv, caps[l], D), dtype), names=("slot", "head", "row", "elem"))
                dec = torch.zeros(B, 1, caps[l], 1, dtype=torch.bool)
                for (_, d), n in zip(pairs, rows):
                    dec[d, :, :n] = True
                a.declare(t, dec)
                lst.append(t)
        snap_k, snap_v = [t.clone() for t in tk], [t.clone() for t in tv]
        L, n = len(layers), max(len(pairs), 1)
        kp = (C.c_void_p * L)(*[t.data_ptr() for t in tk])
        vp = (C.c_void_p * L)(*[t.data_ptr() for t in tv])
        cap = (C.c_int32 * L)(*[caps[l] for l in layers])
        src, dst = (C.c_int32 * n)(*[s for s, _ in pairs]), (C.c_int32 * n)(*[d for _, d in pairs])
        rw = (C.c_int32 * n)(*rows)
        sources = [t[s] for t in tk + tv for s, _ in pairs]
        with frozen(*sources):
            rc = lib.kvz_fork_branch_copy(kp, vp, cap, L, B, Hkv, D, 2, src, dst, rw, len(pairs), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        assert rc == 0, lib.kvz_last_error()
        for t, s0 in zip(tk + tv, snap_k + snap_v):
            for (s, d), r in zip(pairs, rows):
                assert _same(t[d, :, :r], s0[s, :, :r]), (layers, pairs, rows)
        a.assert_clean()


def _hand_base(arena, L, Hkv, G, D, dtype, lens, slack, off):
    """A pruned slack-layout EvictCache whose flat K and V are carved from ``arena`` (None: plain tensors) and keep its pattern."""
    from kvzip_amd.kvcache import EvictCache
    cfg = types.SimpleNamespace(num_hidden_layers=L, num_attention_heads=Hkv * G, num_key_value_heads=Hkv)
    kv = EvictCache(cfg, (0, 100), device=DEV, dtype=dtype, slack=slack, verbose=False)
    starts, totals = [], []
    for l in range(L):
        acc, st = 0, []
        for h in range(Hkv):
            st.append(acc)
            acc += lens[l][h] + slack
        starts.append(st)
        totals.append(acc)
    if arena is not None:
        kv.key_cache = [arena.carve(f"base_k{l}", ((totals[l], D), dtype), names=("row", "elem")) for l in range(L)]
        kv.value_cache = [arena.carve(f"base_v{l}", ((totals[l], D), dtype), names=("row", "elem")) for l in range(L)]
    else:
        g = torch.Generator().manual_seed(7)
        mk = lambda n: torch.randint(-30000, 30000, (n, D), generator=g, dtype=torch.int16).view(dtype).to(DEV)  # noqa: E731
        kv.key_cache, kv.value_cache = [mk(t) for t in totals], [mk(t) for t in totals]
    kv.pruned, kv.get_score, kv._seen_tokens, kv._layout_epoch = True, False, 500 + off, 1
    kv.info = {"flatten": True, "layout": "slack", "cu_head": torch.arange(Hkv + 1, dtype=torch.int32, device=DEV),
               "len_k": [torch.tensor(lens[l], dtype=torch.int32, device=DEV) for l in range(L)], "len_k_host": [list(x) for x in lens],
               "max_len_k": [max(x) for x in lens], "cu_len_k": [None] * L,
               "seg_start": [torch.tensor(starts[l], dtype=torch.int32, device=DEV) for l in range(L)],
               "rows_used": [sum(x) for x in lens], "offset": [off] * L}
    kv._refresh_meta_host()
    return kv, starts


def _fork_with_tails(kv, B, cap, t_len, D, dtype, seed=3):
    fork = kv.fork(B, tail_capacity=cap)
    g = torch.Generator().manual_seed(seed)
    for l in range(kv.n_layers):
        shape = (B, kv.n_heads_kv, cap + 8 * l, D)                     # (capacities may differ between layers)
        fork.tail_k[l] = torch.randint(-30000, 30000, shape, generator=g, dtype=torch.int16).view(dtype).to(DEV)
        fork.tail_v[l] = torch.randint(-30000, 30000, shape, generator=g, dtype=torch.int16).view(dtype).to(DEV)
        fork.tail_len[l] = list(t_len)
    return fork


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_commit_writes_only_the_declared_slack_rows(dtype):
    from kvzip_amd.ops import KvzError
    L, Hkv, G, D, slack, off, B = 2, 3, 2, 128, 16, 2, 3
    lens = [[37, 0, 130], [5, 64, 1]]
    t_len = [4, 11, 0]
    for b in (1, 0, 2):
        a = Arena(DEV)
        kv, starts = _hand_base(a, L, Hkv, G, D, dtype, lens, slack, off)
        t = t_len[b]
        for l in range(L):
            dec = torch.zeros(kv.key_cache[l].shape[0], 1, dtype=torch.bool)
            for h in range(Hkv):
                r0 = starts[l][h] + lens[l][h] + off
                dec[r0:r0 + t] = True
            a.declare(kv.key_cache[l], dec)
            a.declare(kv.value_cache[l], dec)
        fork = _fork_with_tails(kv, B, 12, t_len, D, dtype)
        with frozen(*fork.tail_k, *fork.tail_v, *kv.info["seg_start"], *kv.info["len_k"]):
            fork.commit(b)
            torch.cuda.synchronize()
        assert kv.info["offset"] == [off + t] * L and kv._seen_tokens == 500 + off + t and kv._layout_epoch == 1
        for l in range(L):
            for h in range(Hkv):
                r0 = starts[l][h] + lens[l][h] + off
                assert _same(kv.key_cache[l][r0:r0 + t], fork.tail_k[l][b, h, :t]), (b, l, h)
                assert _same(kv.value_cache[l][r0:r0 + t], fork.tail_v[l][b, h, :t]), (b, l, h)
        a.assert_clean()                                               # the rows the heads held, the free slack, the guards: untouched
        with pytest.raises(KvzError, match="closed"):
            fork.commit(b)


def test_commit_grows_the_slack_first():
    """More rows than the slack has left: the base is re-laid out with a larger slack (its rows move, bit for bit), then appended to."""
    dtype, L, Hkv, G, D, slack, off, B = torch.float16, 2, 2, 2, 64, 4, 2, 2
    lens = [[9, 3], [1, 20]]
    kv, starts = _hand_base(None, L, Hkv, G, D, dtype, lens, slack, off)
    old_k, old_v = [k.clone() for k in kv.key_cache], [v.clone() for v in kv.value_cache]
    fork = _fork_with_tails(kv, B, 8, [5, 3], D, dtype)
    fork.commit(0)
    torch.cuda.synchronize()
    assert kv.slack >= off + 5 and kv._layout_epoch == 2 and kv.info["offset"] == [off + 5] * L and kv._seen_tokens == 500 + off + 5
    for l in range(L):
        new = kv.info["seg_start"][l].tolist()
        for h in range(Hkv):
            n = lens[l][h] + off
            assert _same(kv.key_cache[l][new[h]:new[h] + n], old_k[l][starts[l][h]:starts[l][h] + n])
            assert _same(kv.value_cache[l][new[h]:new[h] + n], old_v[l][starts[l][h]:starts[l][h] + n])
            assert _same(kv.key_cache[l][new[h] + n:new[h] + n + 5], fork.tail_k[l][0, h, :5])
            assert _same(kv.value_cache[l][new[h] + n:new[h] + n + 5], fork.tail_v[l][0, h, :5])
