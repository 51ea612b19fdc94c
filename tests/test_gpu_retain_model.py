"""GPU: RetainCache decoding through its index of kept positions (``indexed=True``, the default) on the tiny random-init Llama of
tests/test_gpu_model.py: several ratios and a level switch on one prefill against a freshly pruned EvictCache and against the gather
route (``indexed=False``), logits bit for bit, the number of gathers per ``generate``, growth of the dense store in the middle of a
generation, the bookkeeping afterwards and a second turn."""
import pytest
import torch

from test_gpu_model import make, prefill_and_score

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_LAYERS = 2


def _retain(indexed=True, **kw):
    m, ctx, rep, query = make("retain", indexed=indexed, **kw)
    return m, prefill_and_score(m, ctx, rep), ctx, rep, query


def _long_query():
    """33 tokens: with the 3 tokens of the template and G = 2 the first step has 72 query rows per KV head - beyond the decode kernels,
    so it gathers and runs the multi-row kernel.  The 14 tokens of the helpers' own query (28 rows) attend through the index."""
    return torch.randint(0, 160, (1, 33), generator=torch.Generator().manual_seed(5))


class _GatherSpy:
    """Counts the calls of ops.compact_plan / compact_layer / compact_layers (what ``RetainCache.prepare`` does per attention call)."""

    def __init__(self, monkeypatch):
        from kvzip_amd import ops
        self.plans = self.gathers = 0
        for name in ("compact_plan", "compact_layer", "compact_layers"):
            orig = getattr(ops, name)

            def spy(*a, _orig=orig, _name=name, **k):
                if _name == "compact_plan":
                    self.plans += 1
                else:
                    self.gathers += 1
                return _orig(*a, **k)
            monkeypatch.setattr(ops, name, spy)

    def reset(self):
        self.plans = self.gathers = 0


def test_flag_reaches_the_cache_and_prune_builds_the_index():
    m, kr, *_ = _retain()
    assert kr.indexed is True and kr._index is None
    kr.prune(0.5)
    ix = kr._index
    assert ix is not None and kr._index_valid is kr.valid and ix.ctx_end == kr.sink + kr.ctx_len == 305
    full = torch.cat([torch.ones(N_LAYERS, 1, 2, 5, dtype=torch.bool, device=DEV), kr.valid], dim=-1)
    assert ix.counts == full.sum(-1)[:, 0].tolist() and ix.total == int(full.sum())
    for l in range(N_LAYERS):
        for h in range(2):
            s, n = ix.starts[l][h], ix.counts[l][h]
            assert torch.equal(ix.idx[s:s + n].long(), torch.nonzero(full[l, 0, h]).flatten())
    kr.prune(0.2)
    assert kr._index is not ix and kr._index.total < ix.total          # a second prune rebuilds it
    m2, k2, *_ = _retain(indexed=False)
    k2.prune(0.5)
    assert k2.indexed is False and k2._index is None


@pytest.mark.parametrize("long_first_step", [False, True], ids=["first-step-indexed", "first-step-gathers"])
def test_ratios_and_level_on_one_prefill(long_first_step):
    """Prune at 0.2, then 0.9, then 0.5, then level pair-uniform, on one prefill: after each, ``generate`` equals a freshly pruned
    EvictCache at that setting and the same cache with ``indexed=False``."""
    m, kr, ctx, rep, query = _retain()
    m0, k0, *_ = _retain(indexed=False)
    me, _, _, _ = make("evict")
    q_ids = m.apply_template(_long_query() if long_first_step else query)
    for ratio, level in ((0.2, "pair"), (0.9, "pair"), (0.5, "pair"), (0.5, "pair-uniform")):
        assert kr.prune(ratio, level) == k0.prune(ratio, level)
        ke = prefill_and_score(me, ctx, rep)
        ke.prune(ratio, level)
        a = m.generate(q_ids, kv=kr, return_ids=True)
        assert torch.equal(a, m0.generate(q_ids, kv=k0, return_ids=True)), (ratio, level, "indexed=False")
        assert torch.equal(a, me.generate(q_ids, kv=ke, return_ids=True)), (ratio, level, "EvictCache")


def test_logits_are_bit_equal_to_the_gather_route():
    """The first step (14 positions through the index) and four single-token forwards: torch.equal logits between indexed=True / False."""
    m, kr, ctx, rep, query = _retain()
    m0, k0, *_ = _retain(indexed=False)
    kr.prune(0.4)
    k0.prune(0.4)
    q_ids = m.apply_template(query)
    g = torch.Generator().manual_seed(2)
    steps = [q_ids] + [torch.randint(0, 160, (1, 1), generator=g).to(DEV) for _ in range(4)]
    for i, ids in enumerate(steps):
        la = m(ids, kr, update_cache=True, return_logits=True).logits
        lb = m0(ids, k0, update_cache=True, return_logits=True).logits
        assert torch.equal(la, lb), (i, float((la.float() - lb.float()).abs().max()))
        assert kr._fill == k0._fill and kr.get_seq_length() == k0.get_seq_length()
        for l in range(N_LAYERS):
            assert kr.key_cache[l].shape == k0.key_cache[l].shape
            assert torch.equal(kr.key_cache[l], k0.key_cache[l]) and torch.equal(kr.value_cache[l], k0.value_cache[l])


def test_gathers_per_generate(monkeypatch):
    """Exactly n_layers gathers per ``generate`` - its first step, when that has more query rows than the decode kernels take - whatever
    the number of decode steps; none when the first step goes through the index too.  The gather route gathers at every call."""
    m, kr, ctx, rep, query = _retain()
    kr.prune(0.4)
    spy = _GatherSpy(monkeypatch)
    long_ids, short_ids = m.apply_template(_long_query()), m.apply_template(query)
    for steps in (2, 6):
        m.gen_kwargs["max_new_tokens"] = steps
        spy.reset()
        m.generate(long_ids, kv=kr, return_ids=True)
        assert (spy.plans, spy.gathers) == (N_LAYERS, N_LAYERS), (steps, spy.plans, spy.gathers)
        spy.reset()
        m.generate(short_ids, kv=kr, return_ids=True)
        assert (spy.plans, spy.gathers) == (0, 0), (steps, spy.plans, spy.gathers)
    m0, k0, *_ = _retain(indexed=False)
    k0.prune(0.4)
    m0.gen_kwargs["max_new_tokens"] = 6
    spy.reset()
    m0.generate(short_ids, kv=k0, return_ids=True)
    assert spy.gathers == 6 * N_LAYERS and spy.plans == 6 * N_LAYERS


def _trim(kv, cap):
    """Cut the dense stores down to `cap` rows per head (prefill grows them by doubling, far beyond reserve)."""
    for l in range(N_LAYERS):
        kv._store_k[l] = kv._store_k[l][:, :, :cap].contiguous()
        kv._store_v[l] = kv._store_v[l][:, :, :cap].contiguous()
    kv._views.clear()
    kv._dense_slice(kv._fill[0])


def test_store_reallocates_mid_generation():
    """reserve=2 (through cache_kwargs) and stores with room for two more rows: the store moves at the first step (several positions,
    ``update``) or - with room for the query and two tokens - at the third single-token step (``update_attend``).  The index holds
    positions, not addresses: the ids are those of a cache that never grows."""
    m, kr, ctx, rep, query = _retain()
    ms, ks, *_ = _retain(reserve=2)
    kr.prune(0.4)
    ks.prune(0.4)
    assert ks._reserve == 2 and ks.indexed
    q_ids = m.apply_template(query)
    m.gen_kwargs["max_new_tokens"] = ms.gen_kwargs["max_new_tokens"] = 8
    a = m.generate(q_ids, kv=kr, return_ids=True)
    grown = []
    orig = ks._dense_grow

    def grow(layer_idx, need):
        before = ks._store_k[layer_idx].shape[2]
        r = orig(layer_idx, need)
        if r[0].shape[2] != before:
            grown.append((layer_idx, need - ks._fill[layer_idx]))
        return r
    ks._dense_grow = grow
    for room, rows in ((2, q_ids.shape[1]), (q_ids.shape[1] + 2, 1)):
        _trim(ks, 305 + room)
        del grown[:]
        b = ms.generate(q_ids, kv=ks, return_ids=True)
        assert grown == [(l, rows) for l in range(N_LAYERS)], (room, grown)     # every layer moved once, for a step of `rows` rows
        assert torch.equal(a, b), room
        assert ks.get_seq_length() == 305 and ks._fill == [305] * N_LAYERS


def test_bookkeeping_after_generate_and_second_generate():
    m, kr, ctx, rep, query = _retain()
    kr.prune(0.3)
    q_ids = m.apply_template(query)
    seen, fill = kr.get_seq_length(), list(kr._fill)
    a = m.generate(q_ids, kv=kr, return_ids=True)
    assert kr.get_seq_length() == seen == 305 and kr._fill == fill
    for l in range(N_LAYERS):
        assert kr.key_cache[l].shape[2] == 305 and kr.value_cache[l].shape[2] == 305
    assert torch.equal(m.generate(q_ids, kv=kr, return_ids=True), a)
    assert kr.get_seq_length() == seen and kr._fill == fill


def test_update_cache_then_second_turn():
    """update_cache=True keeps the rows of query and answer behind the context: every head sees them (computed positions), and a
    second turn equals the gather route's."""
    m, kr, ctx, rep, query = _retain()
    m0, k0, *_ = _retain(indexed=False)
    kr.prune(0.5)
    k0.prune(0.5)
    q_ids = m.apply_template(query)
    seen = kr.get_seq_length()
    a = m.generate(q_ids, kv=kr, update_cache=True, return_ids=True)
    a0 = m0.generate(q_ids, kv=k0, update_cache=True, return_ids=True)
    assert torch.equal(a, a0) and a.shape[1] == 5
    assert kr.get_seq_length() == seen + q_ids.shape[1] + a.shape[1] == k0.get_seq_length()
    assert kr._fill == k0._fill == [kr.get_seq_length()] * N_LAYERS
    b = m.generate(q_ids, kv=kr, return_ids=True)
    assert torch.equal(b, m0.generate(q_ids, kv=k0, return_ids=True))
    assert kr.get_seq_length() == seen + q_ids.shape[1] + a.shape[1]
