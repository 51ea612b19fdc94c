"""GPU: tightening a pruned cache to a smaller ratio without a new prefill (EvictCache.tighten, kvz_recompact_layers,
kvz_mask_resurrects).  The contract is a postcondition: after prune(r1); prune(r2) with r2 <= r1 the cache equals a fresh cache after
prune(r2) - mask, threshold, lengths, segment starts, memory figure and every used row bit for bit; rows appended before the tighten
sit behind each head's rows as if appended after the fresh prune.  Everything here moves bytes or integers: no tolerance anywhere."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16

# three 1024-token tiles, the last partial, three rows behind the context (positions: tile 0 = context 0..1018, tile 1 = 1019..2042)
L, HKV, SINK, N, TAIL = 2, 3, 5, 2 * 1024 + 37, 3
KLEN = SINK + N + TAIL
T1_LO, T1_HI = 1024 - SINK, 2048 - SINK     # context tokens of tile 1


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _tagged(D, dtype, kv_flag, seed):
    """Dense [1, Hkv, klen, D] per layer, every row tagged with (layer, head, position, K / V) in its first four elements."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for l in range(L):
        t = torch.randint(-2 ** 15, 2 ** 15, (1, HKV, KLEN, D), generator=g, dtype=torch.int32)
        t[..., 0] = l
        t[..., 1] = torch.arange(HKV).view(1, HKV, 1)
        t[..., 2] = torch.arange(KLEN).view(1, 1, KLEN)
        t[..., 3] = kv_flag
        out.append(t.to(torch.int16).view(dtype).to(DEV))
    return out


def _full(valid):
    """[L, Hkv, N] bool (CPU) -> full mask [L, Hkv, klen]"""
    return torch.cat([torch.ones(L, HKV, SINK, dtype=torch.bool), valid, torch.ones(L, HKV, TAIL, dtype=torch.bool)], -1)


def _masks(mode, seed):
    """(old, new) as CPU bool [L, Hkv, N] plus the tensors the ops take (token-level [L,1,Hkv,N] or a stride-0 head-level view)."""
    g = torch.Generator().manual_seed(seed)
    if mode == "tok-tok":
        old = torch.rand(L, HKV, N, generator=g) < 0.6
        old[1, 0, T1_LO:T1_HI] = True               # a tile kept entirely by the old mask
        old[1, 1, T1_LO:T1_HI] = False              # a tile emptied by the old mask
        old[1, 2, T1_HI - 1] = True
        new = old & (torch.rand(L, HKV, N, generator=g) < 0.5)
        new[0, 0] = False                           # a head whose new mask is empty
        new[0, 1] = old[0, 1]                       # a head with new == old
        new[1, 2, T1_LO:T1_HI - 1] = False          # a tile whose only new survivor is its last token
        new[1, 2, T1_HI - 1] = True
        assert old[0, 1].any() and not old[0, 1].all() and new[1, 0, T1_LO:T1_HI].any()
        return old, new, old.view(L, 1, HKV, N).to(DEV), new.view(L, 1, HKV, N).to(DEV)
    nh = torch.tensor([[True, False, True], [False, False, True]])
    new = nh.view(L, HKV, 1).expand(L, HKV, N).clone()
    new_t = nh.view(L, 1, HKV, 1).to(DEV).expand(L, 1, HKV, N)
    if mode == "tok-head":                          # the subset holds where the old mask kept every token of the new mask's heads
        old = (torch.rand(L, HKV, N, generator=g) < 0.6) | new
        return old, new, old.view(L, 1, HKV, N).to(DEV), new_t
    oh = nh | torch.tensor([[False, True, False], [False, False, False]])
    old = oh.view(L, HKV, 1).expand(L, HKV, N).clone()
    return old, new, oh.view(L, 1, HKV, 1).to(DEV).expand(L, 1, HKV, N), new_t


def _plan_and_compact(ops, K, V, valid_t, valid_cpu, slack):
    plan = ops.compact_plan(valid_t, SINK, KLEN, slack=slack)
    lens = _full(valid_cpu).sum(-1)
    totals = [int(lens[l].sum()) + HKV * slack for l in range(L)]
    ks, vs = ops.compact_layers(K, V, plan, totals)
    return plan, lens, totals, ks, vs


@pytest.mark.parametrize("mode", ["tok-tok", "tok-head", "head-head"])
@pytest.mark.parametrize("slack", [0, 4])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_recompact_equals_fresh_compaction(D, dtype, slack, mode):
    from kvzip_amd import ops
    K, V = _tagged(D, dtype, 0, seed=D + slack), _tagged(D, dtype, 1, seed=D + slack + 100)
    old, new, old_t, new_t = _masks(mode, seed=slack)
    assert bool((new & ~old).sum() == 0)
    old_plan, old_lens, _, ko, vo = _plan_and_compact(ops, K, V, old_t, old, slack)
    new_plan, new_lens, totals, kf, vf = _plan_and_compact(ops, K, V, new_t, new, slack)
    assert int(ops.mask_resurrects(new_t, old_t)) == 0
    tails = [3, 1] if slack else None
    if tails:    # rows appended after the old prune: behind every head's rows, in its slack
        for l in range(L):
            for h in range(HKV):
                s = int(old_plan.seg_start[l, h]) + int(old_lens[l, h])
                ko[l][s:s + tails[l]] = K[l][0, h, :tails[l]].flip(-1)
                vo[l][s:s + tails[l]] = V[l][0, h, :tails[l]].flip(-1)
    before = [t.clone() for t in ko + vo]
    kr, vr = ops.recompact_layers(ko, vo, old_plan, old_t, new_plan, new_t, totals, tail_rows=tails)
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(before, ko + vo)), "the old flat cache is read only"
    # metadata of the new layout = what the mask says
    assert new_plan.len_k.cpu().tolist() == new_lens.tolist()
    seg = [[int(new_lens[l, :h].sum()) + h * slack for h in range(HKV)] for l in range(L)]
    assert new_plan.seg_start.cpu().tolist() == seg
    full = _full(new)
    for l in range(L):
        assert kr[l].shape == (totals[l], D) and vr[l].shape == (totals[l], D)
        for h in range(HKV):
            s, n = seg[l][h], int(new_lens[l, h])
            idx = full[l, h].nonzero().view(-1).to(DEV)
            for got, fresh, dense in ((kr[l], kf[l], K[l]), (vr[l], vf[l], V[l])):
                assert _same(got[s:s + n], fresh[s:s + n]), (mode, l, h, "recompacted rows != fresh compaction")
                assert _same(got[s:s + n], dense[0, h].index_select(0, idx)), (mode, l, h, "recompacted rows != index_select")
            if tails:
                assert _same(kr[l][s + n:s + n + tails[l]], K[l][0, h, :tails[l]].flip(-1)), (mode, l, h, "appended K rows")
                assert _same(vr[l][s + n:s + n + tails[l]], V[l][0, h, :tails[l]].flip(-1)), (mode, l, h, "appended V rows")


def test_recompact_refuses_appended_rows_beyond_the_slack():
    from kvzip_amd import ops
    K, V = _tagged(64, F16, 0, seed=1), _tagged(64, F16, 1, seed=2)
    old, new, old_t, new_t = _masks("tok-tok", seed=3)
    old_plan, _, _, ko, vo = _plan_and_compact(ops, K, V, old_t, old, 4)
    new_plan, _, totals, _, _ = _plan_and_compact(ops, K, V, new_t, new, 4)
    with pytest.raises(ops.KvzError, match="slack"):
        ops.recompact_layers(ko, vo, old_plan, old_t, new_plan, new_t, totals, tail_rows=[5, 0])


@pytest.mark.parametrize("mode", ["tok-tok", "tok-head", "head-tok", "head-head"])
def test_mask_resurrects_counts_new_only_positions(mode):
    """Unrelated masks: the count is (new & ~old).sum(), for every pairing of token- and head-level masks; odd N (rows unaligned)."""
    from kvzip_amd import ops
    g = torch.Generator().manual_seed(11)

    def mask(level, p, heads):
        if level == "tok":
            m = torch.rand(L, HKV, N, generator=g) < p
            return m, m.view(L, 1, HKV, N).to(DEV)
        mh = torch.tensor(heads)
        return mh.view(L, HKV, 1).expand(L, HKV, N), mh.view(L, 1, HKV, 1).to(DEV).expand(L, 1, HKV, N)
    lo, ln = mode.split("-")
    old, old_t = mask(lo, 0.6, [[True, False, True], [True, False, False]])
    new, new_t = mask(ln, 0.5, [[True, True, False], [False, True, False]])
    want = int((new & ~old).sum())
    assert want > 0
    got = ops.mask_resurrects(new_t, old_t)
    assert got.dtype == torch.int32 and got.is_cuda and int(got) == want
    assert int(ops.mask_resurrects(old_t, old_t)) == 0
    assert int(ops.mask_resurrects(new_t & old_t, old_t)) == 0
    # a single new-only position at the very end of the last row, and N larger than one block's chunk
    big = torch.zeros(1, 1, 2, 4 * 1024 + 3, dtype=torch.bool, device=DEV)
    one = big.clone()
    one[0, 0, 1, -1] = True
    assert int(ops.mask_resurrects(one, big)) == 1 and int(ops.mask_resurrects(big, one)) == 0


# ---- cache level -----------------------------------------------------------------------------------------------------------------
H, D_C = 21, 128     # G = 7


def _cfg():
    return types.SimpleNamespace(num_hidden_layers=L, num_attention_heads=H, num_key_value_heads=HKV)


def _scores(level, dtype):
    g = torch.Generator().manual_seed(21)
    if level == "head":   # as load_head_score returns them: [L, 1, Hkv, N], stride 0 over the context
        hs = torch.tensor([[0.9, 0.2, 0.6], [0.4, 0.8, 0.1]]).to(dtype).to(DEV)
        return hs.unsqueeze(-1).expand(-1, -1, N).unsqueeze(1)
    sc = [torch.rand(1, HKV, N, generator=g).to(dtype) for _ in range(L)]
    sc[0][0, 0] = (torch.rand(N, generator=g) * 8).floor() / 8        # a row of eight distinct values: ties at every boundary
    return [s.to(DEV) for s in sc]


def _cache(level="pair", dtype=F16, layout="slack", slack=8):
    from kvzip_amd.kvcache import EvictCache
    kv = EvictCache(_cfg(), (SINK, SINK + N), device=DEV, dtype=dtype, layout=layout, slack=slack, verbose=False)
    g = torch.Generator().manual_seed(31)      # (finite values: these caches are attended over)
    for l in range(L):
        kv.update(torch.randn(1, HKV, KLEN, D_C, generator=g).to(dtype).to(DEV),
                  torch.randn(1, HKV, KLEN, D_C, generator=g).to(dtype).to(DEV), l)
    kv.score = _scores(level, dtype)
    return kv


def _assert_same_cache(a, b, what):
    """The postcondition: `a` (tightened) holds what `b` (freshly pruned) holds."""
    assert torch.equal(a.valid, b.valid) and a.valid.shape == b.valid.shape and a.valid.stride() == b.valid.stride(), what
    assert a._evicted == b._evicted and a._mem() == b._mem() and a.pruned and a.info["flatten"], what
    for key in ("len_k_host", "max_len_k", "rows_used", "offset", "layout"):
        assert a.info[key] == b.info[key], (what, key)
    assert a._seen_tokens == b._seen_tokens
    for l in range(L):
        for key in ("len_k", "seg_start", "cu_len_k"):
            assert torch.equal(a.info[key][l], b.info[key][l]), (what, key, l)
        assert a.key_cache[l].shape == b.key_cache[l].shape and a.value_cache[l].shape == b.value_cache[l].shape, what
        seg = b.info["seg_start"][l].tolist()
        for h in range(HKV):
            n = b.info["len_k_host"][l][h] + b.info["offset"][l]
            assert _same(a.key_cache[l][seg[h]:seg[h] + n], b.key_cache[l][seg[h]:seg[h] + n]), (what, "K", l, h)
            assert _same(a.value_cache[l][seg[h]:seg[h] + n], b.value_cache[l][seg[h]:seg[h] + n]), (what, "V", l, h)
    if a.layout == "slack":
        assert [list(m) for m in a.info["meta_host"]] == [list(m) for m in b.info["meta_host"]], what
    else:
        assert a.info["meta_host"] is None and b.info["meta_host"] is None


@pytest.mark.parametrize("layout", ["slack", "packed"])
@pytest.mark.parametrize("level", ["pair", "pair-uniform", "head"])
def test_chain_of_ratios_equals_fresh_prunes(level, layout):
    kv = _cache(level, layout=layout)
    epoch = kv._layout_epoch
    kept = []
    for ratio in (0.9, 0.6, 0.3, 0.1):
        got = kv.prune(ratio, level)
        fresh = _cache(level, layout=layout)
        want = fresh.prune(ratio, level)
        assert got == want, (level, ratio, got, want)
        epoch += 1
        assert kv._layout_epoch == epoch
        _assert_same_cache(kv, fresh, (level, layout, ratio))
        kept.append(sum(kv.info["rows_used"]))
    assert kept[0] > kept[1] > kept[2] > kept[3], kept     # every link really evicted something
    # tighten() by name, at the ratio the cache already has: a copy of itself
    got = kv.tighten(0.1, level)
    assert got == want
    _assert_same_cache(kv, fresh, (level, layout, "0.1 again"))


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_bf16_and_f16_scores_tighten_alike(dtype):
    kv, fresh = _cache("pair", dtype=dtype), _cache("pair", dtype=dtype)
    kv.prune(0.7)
    assert kv.prune(0.25) == fresh.prune(0.25)
    _assert_same_cache(kv, fresh, str(dtype))


def _attn_probe(kv, q):
    """Attention of layer 0 over the cache as it stands (changes nothing)."""
    from kvzip_amd import ops
    lens = kv.info["len_k"][0] + kv.info["offset"][0]
    return ops.varlen_attn(q, kv.key_cache[0], kv.value_cache[0], kv.info["seg_start"][0], lens.int(), 1,
                           kv.info["max_len_k"][0] + kv.info["offset"][0])


def _randn_like_states(g, dtype, t):
    q = torch.randn(1, H, t, D_C, generator=g).to(dtype).to(DEV)
    k = torch.randn(1, HKV, t, D_C, generator=g).to(dtype).to(DEV)
    v = torch.randn(1, HKV, t, D_C, generator=g).to(dtype).to(DEV)
    return q, k, v


@pytest.mark.parametrize("level", ["pair", "pair-uniform", "head"])
def test_a_larger_ratio_raises_and_changes_nothing(level):
    kv = _cache(level)
    kv.prune(0.3, level)
    g = torch.Generator().manual_seed(41)
    q = torch.randn(HKV, H // HKV, D_C, generator=g).half().to(DEV)
    valid, valid_copy, evicted, epoch = kv.valid, kv.valid.clone(), kv._evicted, kv._layout_epoch
    info, plan = kv.info, kv._plan
    ptrs = [t.data_ptr() for t in kv.key_cache + kv.value_cache]
    rows = [t.clone() for t in kv.key_cache + kv.value_cache]
    out = _attn_probe(kv, q)
    with pytest.raises(ValueError, match="evicted"):
        kv.prune(0.5, level)
    assert kv.valid is valid and torch.equal(kv.valid, valid_copy) and kv._evicted == evicted
    assert kv.info is info and kv._plan is plan and kv._layout_epoch == epoch and kv.pruned
    assert [t.data_ptr() for t in kv.key_cache + kv.value_cache] == ptrs
    assert all(_same(a, b) for a, b in zip(rows, kv.key_cache + kv.value_cache))
    assert _same(out, _attn_probe(kv, q))
    fresh = _cache(level)
    assert kv.prune(0.2, level) == fresh.prune(0.2, level)     # and the cache still tightens
    _assert_same_cache(kv, fresh, (level, "after the refused request"))


def test_mixed_levels_that_are_not_nested_raise():
    kv = _cache("pair")
    kv.prune(0.5, "pair")
    with pytest.raises(ValueError, match="evicted"):
        kv.prune(0.5, "pair-uniform")       # (half of every row, of a cache cut at the global median: some row needs pairs back)


def _append(kv, g, dtype, t):
    for l in range(L):
        q, k, v = _randn_like_states(g, dtype, t)
        ke, ve = kv.update(k, v, l)
        kv.prepare(q, ke, ve, l)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_appended_rows_follow_the_tightened_heads(dtype):
    """prune, append t = 3 then t = 1 per layer, tighten == fresh prune at the small ratio, then the same appends; one decode step."""
    a, b = _cache(dtype=dtype), _cache(dtype=dtype)
    ga, gb = torch.Generator().manual_seed(51), torch.Generator().manual_seed(51)
    a.prune(0.6)
    _append(a, ga, dtype, 3)
    _append(a, ga, dtype, 1)
    assert a.info["offset"] == [4] * L
    assert a.prune(0.3) == b.prune(0.3)
    assert a.info["offset"] == [4] * L
    _append(b, gb, dtype, 3)
    _append(b, gb, dtype, 1)
    _assert_same_cache(a, b, "appended rows")
    for l in range(L):
        q, k, v = _randn_like_states(ga, dtype, 1)
        assert _same(a.update_attend(q, k, v, l), b.update_attend(q, k, v, l)), l
    assert a.info["offset"] == [5] * L
    _assert_same_cache(a, b, "after a decode step")
    seen = a._seen_tokens - 5
    a.slice(seen); b.slice(seen)
    _assert_same_cache(a, b, "after slice")


def test_tighten_after_the_slack_grew():
    """More rows appended than the slack held: the segments moved since the prune; the tighten reads them where they are."""
    a = _cache(slack=2)
    g = torch.Generator().manual_seed(61)
    a.prune(0.6)
    _append(a, g, F16, 3)
    assert a.slack > 2
    b = _cache(slack=a.slack)
    g = torch.Generator().manual_seed(61)
    assert a.prune(0.3) == b.prune(0.3)
    _append(b, g, F16, 3)
    _assert_same_cache(a, b, "grown slack")


def test_packed_layout_with_appended_rows_is_refused():
    from kvzip_amd import ops
    kv = _cache(layout="packed")
    kv.prune(0.6)
    seen = kv._seen_tokens
    _append(kv, torch.Generator().manual_seed(71), F16, 2)
    with pytest.raises(ops.KvzError, match="packed"):
        kv.prune(0.3)
    kv.slice(seen)
    fresh = _cache(layout="packed")
    assert kv.prune(0.3) == fresh.prune(0.3)
    _assert_same_cache(kv, fresh, "packed after slice")


def test_tighten_needs_a_pruned_cache():
    from kvzip_amd import ops
    with pytest.raises(ops.KvzError, match="not pruned"):
        _cache().tighten(0.3)


def test_stale_fork_and_decode_graph_raise_new_ones_work():
    from kvzip_amd import ops
    kv = _cache(slack=16)
    kv.prune(0.6)
    g = torch.Generator().manual_seed(81)
    q2 = torch.randn(2, H, 1, D_C, generator=g).half().to(DEV)
    k2 = torch.randn(2, HKV, 1, D_C, generator=g).half().to(DEV)
    qb = torch.randn(L, 1, H, 1, D_C, generator=g).half().to(DEV)
    kb = torch.randn(L, 1, HKV, 1, D_C, generator=g).half().to(DEV)
    fork = kv.fork(2)
    fork.update_attend(q2, k2, k2, 0)
    graph = kv.decode_graph(qb, kb, kb)
    graph.replay()
    kv.slice(kv._seen_tokens - 1)
    kv.prune(0.3)
    with pytest.raises(ops.KvzError, match="re-laid out"):
        fork.update_attend(q2, k2, k2, 0)
    with pytest.raises(ops.KvzError, match="re-laid out"):
        fork.first_step(q2[:1], k2[:1], k2[:1], 0)
    with pytest.raises(ops.KvzError, match="re-laid out"):
        graph.replay()
    fork2 = kv.fork(2)                       # a new fork and a new graph of the new layout work
    fork2.update_attend(q2, k2, k2, 0)
    fresh = _cache(slack=16)
    fresh.prune(0.3)
    want = torch.stack([fresh.update_attend(qb[l], kb[l], kb[l], l) for l in range(L)])
    got = kv.decode_graph(qb, kb, kb).replay()
    assert _same(got, want)


# ---- model level -----------------------------------------------------------------------------------------------------------------
def test_generate_after_a_tighten_equals_generate_after_a_fresh_prune():
    from test_gpu_model import make, prefill_and_score
    m, ctx, rep, query = make("evict")
    q_ids = m.apply_template(query)
    kv = prefill_and_score(m, ctx, rep)
    kv.prune(0.6)
    first = m.generate(q_ids, kv=kv, return_ids=True)
    got_r = kv.prune(0.3)
    fresh = prefill_and_score(m, ctx, rep)
    assert fresh.prune(0.3) == got_r
    assert torch.equal(kv.valid, fresh.valid) and kv.info["len_k_host"] == fresh.info["len_k_host"]
    want = m.generate(q_ids, kv=fresh, return_ids=True)
    got = m.generate(q_ids, kv=kv, return_ids=True)
    assert torch.equal(got, want) and first.shape[0] == 1
    # multi-turn: the first turn's K,V stay in the cache across the tighten
    a, b = prefill_and_score(m, ctx, rep), prefill_and_score(m, ctx, rep)
    a.prune(0.6)
    turn_a = m.generate(q_ids, kv=a, update_cache=True, return_ids=True)
    assert a.info["offset"][0] > 0
    a.prune(0.6)                             # (same ratio: the layout is rebuilt, every row stays)
    b.prune(0.6)
    turn_b = m.generate(q_ids, kv=b, update_cache=True, return_ids=True)
    assert torch.equal(turn_a, turn_b) and a.info["offset"] == b.info["offset"]
    assert torch.equal(m.generate(q_ids, kv=a, return_ids=True), m.generate(q_ids, kv=b, return_ids=True))


def test_eval_ratios_evict_gives_the_records_of_eval_ratios():
    from test_gpu_model import make, prefill_and_score
    ratios = [0.9, 0.5, 0.2]
    m, ctx, rep, query = make("retain")
    kr = prefill_and_score(m, ctx, rep)
    q_ids = m.apply_template(query)
    want = m.eval_ratios(kr, ratios, lambda kv: m.generate(q_ids, kv=kv, return_ids=True))
    m2, _, _, _ = make("evict")
    ke = prefill_and_score(m2, ctx, rep)
    mem = []

    def fn(kv):
        mem.append(sum(kv.info["rows_used"]))
        return m2.generate(q_ids, kv=kv, return_ids=True)
    got = m2.eval_ratios_evict(ke, ratios, fn)
    assert [r for r, _ in got] == [r for r, _ in want]
    for (_, a), (_, b) in zip(got, want):
        assert torch.equal(a, b)
    assert mem[0] > mem[1] > mem[2]          # the evicting cache really shrank between the evaluations
    with pytest.raises(ValueError, match="non-increasing"):
        m2.eval_ratios_evict(ke, [0.1, 0.2], fn)
    assert len(mem) == 3
