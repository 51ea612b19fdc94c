"""CPU: the host side of tree speculative decoding - ancestor masks (kvzip_amd/ops.py), the prompt-lookup tree drafter and the greedy
tree acceptance (kvzip_amd/draft.py), the tree branch of the speculative loop on a scripted model (kvzip_amd/wrapper.py) and the
refusals of EvictCache.keep_path."""
import random
import types

import pytest
import torch

from kvzip_amd import ops
from kvzip_amd.draft import accept_tree_greedy, lookup_draft, lookup_tree


def ids(*x):
    return torch.tensor(x, dtype=torch.long)


# ---- ancestor masks ------------------------------------------------------------------------------------------------------------------
def _ancestors(parents, p):
    out = set()
    while p >= 0:
        out.add(p)
        p = parents[p]
    return out


def test_ancestor_masks_chain_star_random():
    assert ops.ancestor_masks([]) == []
    assert ops.ancestor_masks([-1]) == [1]
    assert ops.ancestor_masks([-1, 0, 1, 2]) == [0b1, 0b11, 0b111, 0b1111]                       # chain: bits 0 .. p
    assert ops.ancestor_masks([-1, 0, 0, 0]) == [0b1, 0b11, 0b101, 0b1001]                       # star: the root and itself
    assert ops.ancestor_masks([-1, 0, 0, 1, 2]) == [0b1, 0b11, 0b101, 0b1011, 0b10101]           # two interleaved chains
    rng = random.Random(0)
    for t in (2, 7, 33, 64):
        parents = [-1] + [rng.randrange(i) for i in range(1, t)]
        masks = ops.ancestor_masks(parents)
        for p in range(t):
            assert masks[p] == sum(1 << j for j in _ancestors(parents, p)), (t, p)
            assert (masks[p] >> p) & 1 and masks[p] >> (p + 1) == 0


def test_ancestor_masks_at_64_nodes_use_bit_63_and_nothing_above():
    chain = ops.ancestor_masks([-1] + list(range(63)))
    assert chain[63] == (1 << 64) - 1 and chain[62] == (1 << 63) - 1
    star = ops.ancestor_masks([-1] + [0] * 63)
    assert star[63] == (1 << 63) | 1
    assert all(0 < m < (1 << 64) for m in chain + star)


def test_ancestor_masks_refuse_what_is_no_tree_in_topological_order():
    for bad in ([0], [-1, 1], [-1, 0, 2], [-1, -1], [-1, 0, 5], [-1] + list(range(64))):
        with pytest.raises(ops.KvzError, match="ancestor_masks"):
            ops.ancestor_masks(bad)


# ---- lookup_tree ---------------------------------------------------------------------------------------------------------------------
def test_one_occurrence_is_lookup_drafts_chain():
    for h in (ids(1, 2, 3, 50, 51, 52, 9, 1, 2, 3), ids(4, 5, 6, 4, 5), ids(3, 3), ids(7, 8, 7, 8)):
        for n in (1, 2, 3, 8):
            for kw in ({}, {"ngram_max": 1}, {"ngram_max": 5}):
                t_ids, parents = lookup_tree(h, n, max_branches=1, **kw)
                want = lookup_draft(h, n, **kw)
                assert t_ids.tolist() == want.tolist() and parents == list(range(len(parents))), (h.tolist(), n, kw)
                assert t_ids.dtype == torch.long and t_ids.dim() == 1
    # several branches allowed, one occurrence there: still the chain
    h = ids(1, 2, 3, 50, 51, 52, 9, 1, 2, 3)
    t_ids, parents = lookup_tree(h, 3)
    assert t_ids.tolist() == [50, 51, 52] and parents == [0, 1, 2]


def test_two_occurrences_with_a_shared_first_token_merge():
    #         (1 2) 30 40 .. (1 2) 30 41 .. (1 2)
    h = ids(1, 2, 30, 40, 9, 1, 2, 30, 41, 8, 1, 2)
    t_ids, parents = lookup_tree(h, 8, ngram_max=2, ngram_min=2)
    # latest occurrence: 30 41 8 1 2; the earlier: 30 40 9 1 2 30 41 8 -> one node 30, then two children, the latest's first
    assert t_ids.tolist()[:2] == [30, 41] and parents[:2] == [0, 1]
    assert t_ids.tolist().count(30) == 1 or parents[t_ids.tolist().index(30, 1)] != 0     # ONE first-level node 30
    first_level = [i for i, p in enumerate(parents) if p == 0]
    assert first_level == [0]
    kids_of_30 = [t_ids[i].item() for i, p in enumerate(parents) if p == 1]
    assert kids_of_30 == [41, 40]                                                          # latest first
    assert len(parents) == 8 and all(p <= i for i, p in enumerate(parents))                # parents precede children (node i + 1)


def test_budget_is_dealt_breadth_first_and_latest_first():
    #       (7) 10 11 12 .. (7) 20 21 22 .. (7) 30 31 32 .. (7)
    h = ids(7, 10, 11, 12, 0, 7, 20, 21, 22, 0, 7, 30, 31, 32, 0, 7)
    t_ids, parents = lookup_tree(h, 3, ngram_max=1)
    assert t_ids.tolist() == [30, 20, 10] and parents == [0, 0, 0]                         # depth 1 of every occurrence, latest first
    t_ids, parents = lookup_tree(h, 4, ngram_max=1)
    assert t_ids.tolist() == [30, 31, 20, 10] and parents == [0, 1, 0, 0]                  # the 4th node deepens the latest; depth-first order
    t_ids, parents = lookup_tree(h, 6, ngram_max=1)
    assert t_ids.tolist() == [30, 31, 20, 21, 10, 11] and parents == [0, 1, 0, 3, 0, 5]
    t_ids, parents = lookup_tree(h, 2, ngram_max=1)
    assert t_ids.tolist() == [30, 20] and parents == [0, 0]
    t_ids, parents = lookup_tree(h, 4, ngram_max=1, max_branches=2)
    assert t_ids.tolist() == [30, 31, 20, 21] and parents == [0, 1, 0, 3]
    # deterministic
    a, b = lookup_tree(h, 6, ngram_max=1), lookup_tree(h, 6, ngram_max=1)
    assert a[0].tolist() == b[0].tolist() and a[1] == b[1]


def test_continuation_that_runs_into_the_end_is_shorter():
    h = ids(4, 5, 6, 4, 5)
    t_ids, parents = lookup_tree(h, 8)
    assert t_ids.tolist() == [6, 4, 5] and parents == [0, 1, 2]


def test_no_match_gives_an_empty_tree():
    for h, kw in ((ids(1, 2, 3, 4, 5), {}), (ids(), {}), (ids(7), {}), (ids(1, 2, 3), {"ngram_max": 3, "ngram_min": 3})):
        t_ids, parents = lookup_tree(h, 4, **kw)
        assert t_ids.numel() == 0 and t_ids.dim() == 1 and parents == []
    t_ids, parents = lookup_tree(ids(1, 2, 1), 0)
    assert t_ids.numel() == 0 and parents == []


def test_long_history():
    g = torch.Generator().manual_seed(0)
    h = torch.randint(100, 50000, (131072,), generator=g)
    h[1000:1005] = torch.tensor([11, 12, 13, 14, 15])
    h[70000:70005] = torch.tensor([11, 12, 13, 14, 16])
    h[-3:] = torch.tensor([11, 12, 13])
    t_ids, parents = lookup_tree(h, 3)
    assert t_ids.tolist() == [14, 16, 15] and parents == [0, 1, 1]


# ---- accept_tree_greedy ----------------------------------------------------------------------------------------------------------------
def test_accept_tree_greedy():
    # nodes: 0 root; 1: 5 (p0); 2: 6 (p1); 3: 9 (p1); 4: 7 (p0); 5: 8 (p4)
    t_ids, parents = ids(5, 6, 9, 7, 8), [0, 1, 1, 0, 4]
    assert accept_tree_greedy(t_ids, parents, ids(5, 6, 0, 0, 0, 0)) == [0, 1, 2]          # first child, twice: full depth
    assert accept_tree_greedy(t_ids, parents, ids(5, 9, 0, 0, 0, 0)) == [0, 1, 3]          # a later sibling at depth 2
    assert accept_tree_greedy(t_ids, parents, ids(7, 0, 0, 0, 8, 0)) == [0, 4, 5]          # a later sibling at depth 1, then its child
    assert accept_tree_greedy(t_ids, parents, ids(7, 6, 0, 0, 3, 0)) == [0, 4]             # (argmax at node 1 is not on the path)
    assert accept_tree_greedy(t_ids, parents, ids(3, 6, 6, 6, 8, 8)) == [0]                # stop at depth 0
    assert accept_tree_greedy(ids(), [], ids(4)) == [0]
    assert accept_tree_greedy(t_ids, torch.tensor(parents), ids(5, 6, 0, 0, 0, 0)) == [0, 1, 2]


# ---- the tree loop on a scripted model (host logic only: no attention runs) --------------------------------------------------------------
V = 50
WRONG = V - 1


def _scripted(monkeypatch, max_new_tokens=12, eos=None):
    """A ModelKVzip whose "model" is a deterministic function of the ids on the path to a node, over an EvictCache that only keeps the
    books; ops.tree_keep_path is replaced by the same move on the books."""
    import ctypes as C
    from kvzip_amd.kvcache import EvictCache
    from kvzip_amd.wrapper import ModelKVzip
    cfg = types.SimpleNamespace(num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2)

    class Books(EvictCache):
        def slice(self, seen):
            del self.fed[len(self.fed) - (self._seen_tokens - seen):]
            super().slice(seen)

        def rewind(self, n):
            super().rewind(n)
            del self.fed[len(self.fed) - n:]

    kv = Books(cfg, (0, 16), device="cpu", dtype=torch.float16, verbose=False)
    kv.pruned = True
    kv.info = {"flatten": True, "layout": "slack", "offset": [0, 0], "len_k_host": [[4, 6], [5, 3]],
               "meta_host": [(C.c_int32 * 4)(0, 100, 4, 6), (C.c_int32 * 4)(0, 200, 5, 3)]}
    kv.key_cache, kv.value_cache = ["k0", "k1"], ["v0", "v1"]
    kv._seen_tokens = 16
    kv.fed = list(range(16))
    kv.prefill_ids = torch.arange(16)[None]
    calls, moves = [], []

    def fake_keep(k_caches, v_caches, row0, path, t):
        off = kv.info["offset"][0]
        assert list(k_caches) == ["k0", "k1"] and list(v_caches) == ["v0", "v1"]
        assert list(row0) == [4 + off - t, 106 + off - t, 5 + off - t, 203 + off - t]     # start + kept rows + positions before the step
        assert any(p != i for i, p in enumerate(path))                                    # (an identity path launches nothing)
        tail = kv.fed[len(kv.fed) - t:]
        for i, p in enumerate(path):
            kv.fed[len(kv.fed) - t + i] = tail[p]
        moves.append(list(path))
    monkeypatch.setattr(ops, "tree_keep_path", fake_keep)

    def model(ids, past_key_values=None, use_cache=True, position_ids=None):
        kv = past_key_values
        t = ids.shape[1]
        anc = getattr(kv, "_verify_anc", None)
        calls.append((t, bool(getattr(kv, "_verifying", False)), anc is not None))
        toks = ids[0].tolist()
        if anc is None:
            anc = [(1 << (p + 1)) - 1 for p in range(t)]
        assert len(anc) == t
        if position_ids is not None:
            assert position_ids[0].tolist() == [kv._seen_tokens + bin(m).count("1") - 1 for m in anc]
        logits = torch.zeros(1, t, V)
        for i in range(t):
            seen = kv.fed + [toks[j] for j in range(i + 1) if (anc[i] >> j) & 1]
            # (a short period so that prompt lookup finds something to quote)
            logits[0, i, (3 * seen[-1] + seen[-2] + len(seen) % 2) % 7] = 1.0
        kv.fed += toks
        kv._seen_tokens += t
        kv.info["offset"] = [o + t for o in kv.info["offset"]]
        return types.SimpleNamespace(logits=logits)

    m = ModelKVzip.__new__(ModelKVzip)
    m.device, m.config, m.model, m.tokenizer = torch.device("cpu"), cfg, model, None
    m.gen_kwargs = {"do_sample": False, "max_new_tokens": max_new_tokens}
    if eos is not None:
        m.gen_kwargs["eos_token_id"] = eos
    m.sample_generator = None
    return m, kv, calls, moves


def _gen(m, *a, **k):
    from kvzip_amd.wrapper import ModelKVzip
    return ModelKVzip.generate.__wrapped__.__wrapped__(m, *a, **k)


def _spec(m, *a, **k):
    from kvzip_amd.wrapper import ModelKVzip
    return ModelKVzip.generate_speculative.__wrapped__.__wrapped__(m, *a, **k)


def second_sibling(full):
    """A drafter that knows the answer and puts the right token SECOND among two siblings at every depth: n // 2 levels of (wrong,
    right), the next level under the right one.  Nodes depth-first: wrong (a leaf), right, its wrong child, its right child, ..."""
    def draft(h, n):
        done = h.shape[0] - 19                       # ids of `full` the history holds
        right = full[done:done + n // 2]
        t_ids, parents = [], []
        for lvl, tok in enumerate(right):
            t_ids += [WRONG, tok]
            parents += [2 * lvl, 2 * lvl]            # both continue the previous level's right node (0: the root)
        return torch.tensor(t_ids, dtype=torch.long), parents
    return draft


def first_chain(full):
    """What a chain drafter makes of the same proposals: the first child at every level - the wrong one."""
    return lambda h, n: torch.full((min(n, 1),), WRONG, dtype=torch.long)


def test_tree_loop_on_a_scripted_model(monkeypatch):
    """Same ids as generate for every drafter, budget and answer length; the cache's books end where generate leaves them."""
    q = torch.tensor([[5, 1, 4]])
    for max_new in (1, 2, 3, 7, 12):
        m, kv, _, _ = _scripted(monkeypatch, max_new)
        full = _gen(m, q, kv=kv, return_ids=True)[0].tolist()
        assert len(full) == max_new - 1
        drafters = {
            "lookup": None,
            "second sibling": second_sibling(full),
            "right chain": lambda h, n: (torch.tensor(full[h.shape[0] - 19:h.shape[0] - 19 + n], dtype=torch.long),
                                         list(range(len(full[h.shape[0] - 19:h.shape[0] - 19 + n])))),
            "wrong star": lambda h, n: (torch.full((n,), WRONG, dtype=torch.long), [0] * n),
            "too many": lambda h, n: (torch.full((n + 5,), WRONG, dtype=torch.long), [0] * (n + 5)),
            "empty": lambda h, n: (torch.zeros(0, dtype=torch.long), []),
        }
        for name, d in drafters.items():
            for nd in (None, 1, 4, 100):
                m, kv, calls, _ = _scripted(monkeypatch, max_new)
                out, st = _spec(m, q, kv, draft=d, num_draft=nd, return_ids=True, return_stats=True, tree=True)
                assert out[0].tolist() == full, (max_new, name, nd)
                assert kv._seen_tokens == 16 and kv.info["offset"] == [0, 0] and kv.fed == list(range(16)), (max_new, name, nd)
                assert st["tokens"] == max_new - 1 and st["accepted"] <= st["drafted"] and st["steps"] <= st["tokens"]
                assert st["nodes"] == sum(t for t, _, tr in calls[1:] if tr)
                assert all(v == tr == (t > 1) for t, v, tr in calls[1:]) and calls[0] == (3, False, False)
                assert all(t <= 1 + m._draft_len(nd) for t, _, _ in calls[1:])
                if name in ("wrong star", "too many"):
                    assert st["accepted"] == 0 and st["steps"] == st["tokens"]
                if name == "empty":
                    assert st["drafted"] == 0 and all(t == 1 for t, _, _ in calls[1:]) and st["nodes"] == 0
                if name == "right chain" and max_new > 2:
                    assert st["accepted"] == st["drafted"] > 0 and st["steps"] < st["tokens"]
                # update_cache=True: the query and the answer stay, as after generate
                m, kv, _, _ = _scripted(monkeypatch, max_new)
                _spec(m, q, kv, draft=d, num_draft=nd, update_cache=True, tree=True)
                m2, kv2, _, _ = _scripted(monkeypatch, max_new)
                _gen(m2, q, kv=kv2, update_cache=True)
                assert kv.fed == kv2.fed == list(range(16)) + [5, 1, 4] + full and kv._seen_tokens == kv2._seen_tokens
                assert kv.info["offset"] == kv2.info["offset"] and torch.equal(kv.prefill_ids, kv2.prefill_ids)


def test_tree_loop_counts_with_the_right_token_as_second_sibling(monkeypatch):
    """Steps, tokens, drafted, accepted and nodes are EXACTLY what the drafter's shape predicts; the chain form with the first chain of
    the same proposals (the wrong sibling) needs one forward per token."""
    q = torch.tensor([[5, 1, 4]])
    for max_new in (2, 7, 12, 30):
        m, kv, _, _ = _scripted(monkeypatch, max_new)
        full = _gen(m, q, kv=kv, return_ids=True)[0].tolist()
        for nd in (None, 1, 2, 5, 100):
            m, kv, calls, moves = _scripted(monkeypatch, max_new)
            budget = m._draft_len(nd)
            # the prediction: a step with room r asks for n = min(budget, r - 1) nodes, gets n // 2 levels, all accepted
            want = {"steps": 0, "tokens": 0, "drafted": 0, "accepted": 0, "nodes": 0}
            have, want_moves = 1, []
            while have < max_new:
                n = min(budget, max_new - have - 1)
                lv = n // 2
                want["steps"] += 1
                want["tokens"] += lv + 1
                want["drafted"] += 2 * lv
                want["accepted"] += lv
                want["nodes"] += 2 * lv + 1 if lv else 0
                if lv:
                    want_moves.append([0] + [2 * i + 2 for i in range(lv)])
                have += lv + 1
            out, st = _spec(m, q, kv, draft=second_sibling(full), num_draft=nd, return_ids=True, return_stats=True, tree=True)
            assert out[0].tolist() == full and st == want, (max_new, nd, st, want)
            assert moves == want_moves
            assert kv.fed == list(range(16)) and kv.info["offset"] == [0, 0]
            m, kv, _, _ = _scripted(monkeypatch, max_new)
            out, st_chain = _spec(m, q, kv, draft=first_chain(full), num_draft=nd, return_ids=True, return_stats=True)
            assert out[0].tolist() == full and st_chain["steps"] == st_chain["tokens"] == max_new - 1
            assert st["steps"] <= st_chain["steps"] and (budget < 2 or max_new < 4 or st["steps"] < st_chain["steps"])


def test_tree_loop_stops_at_eos_like_generate(monkeypatch):
    q = torch.tensor([[5, 1, 4]])
    m, kv, _, _ = _scripted(monkeypatch, 12)
    full = _gen(m, q, kv=kv, return_ids=True)[0].tolist()
    for eos in sorted(set(full)):
        m, kv, _, _ = _scripted(monkeypatch, 12, eos=eos)
        want = _gen(m, q, kv=kv, return_ids=True)[0].tolist()
        assert want == full[:full.index(eos)]
        for d in (None, second_sibling(full)):
            for nd in (2, 3, 100):
                m, kv, _, _ = _scripted(monkeypatch, 12, eos=eos)
                assert _spec(m, q, kv, draft=d, num_draft=nd, return_ids=True, tree=True)[0].tolist() == want
                assert kv.fed == list(range(16)) and kv.info["offset"] == [0, 0]
                _spec(m, q, kv, draft=d, num_draft=nd, update_cache=True, tree=True)
                assert kv.fed == list(range(16)) + [5, 1, 4] + want and kv.info["offset"] == [3 + len(want)] * 2


def test_tree_form_keeps_the_refusals_of_the_chain_form():
    from kvzip_amd.kvcache import EvictCache
    from kvzip_amd.wrapper import ModelKVzip
    m = ModelKVzip.__new__(ModelKVzip)
    m.device = torch.device("cpu")
    m.config = types.SimpleNamespace(num_hidden_layers=2, num_attention_heads=28, num_key_value_heads=4)
    fn = ModelKVzip.generate_speculative.__wrapped__.__wrapped__
    m.gen_kwargs = {"do_sample": True}
    with pytest.raises(ValueError, match="greedy"):
        fn(m, torch.zeros(1, 3, dtype=torch.long), None, tree=True)
    m.gen_kwargs = {"do_sample": False, "max_new_tokens": 4}
    dense = EvictCache(m.config, (0, 16), device="cpu", dtype=torch.float16, verbose=False)
    with pytest.raises(ValueError, match="use generate"):
        fn(m, torch.zeros(1, 3, dtype=torch.long), dense, tree=True)


# ---- EvictCache.keep_path / verifying(tree=...) on a CPU cache object -----------------------------------------------------------------
def _cache(layout="slack", pruned=True, offset=(5, 5)):
    from kvzip_amd.kvcache import EvictCache
    cfg = types.SimpleNamespace(num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2)
    kv = EvictCache(cfg, (0, 16), device="cpu", dtype=torch.float16, layout=layout, verbose=False)
    if pruned:
        kv.pruned = True
        kv.info = {"flatten": True, "layout": layout, "offset": list(offset)}
        kv._seen_tokens = 16 + offset[0]
    return kv


def test_keep_path_refusals_touch_nothing(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("keep_path launched although it had to refuse")
    monkeypatch.setattr(ops, "tree_keep_path", no_launch)
    with pytest.raises(ops.KvzError, match="slack-layout"):
        _cache(layout="packed").keep_path([0, 2], 3)
    with pytest.raises(ops.KvzError, match="slack-layout"):
        _cache(pruned=False).keep_path([0, 2], 3)
    kv = _cache(offset=(5, 4))
    with pytest.raises(ops.KvzError, match="between forward passes"):
        kv.keep_path([0, 2], 3)
    assert kv.info["offset"] == [5, 4]
    kv = _cache()
    for path, t, what in (([0, 2], 6, "t = 6"), ([0, 2], 0, "t = 0"), ([0, 2], 65, "t = 65"), ([0, 3], 3, r"path\[1\] = 3"),
                          ([2, 1], 4, r"path\[1\] = 1"), ([0, 1, 1], 4, r"path\[2\] = 1"), ([0, 0], 4, r"path\[1\] = 0"),
                          ([-1, 2], 4, r"path\[0\] = -1"), ([0, 1, 2, 3, 4], 4, r"path\[4\] = 4")):
        with pytest.raises(ops.KvzError, match=what):
            kv.keep_path(path, t)
        assert kv.info["offset"] == [5, 5] and kv._seen_tokens == 21
    # an identity path is host bookkeeping alone: no launch, the rest of the t positions taken back
    kv.keep_path([0, 1], 4)
    assert kv.info["offset"] == [3, 3] and kv._seen_tokens == 19
    kv.keep_path([], 3)
    assert kv.info["offset"] == [0, 0] and kv._seen_tokens == 16


def test_verifying_with_a_tree_sets_the_masks_only_inside():
    kv = _cache()
    assert getattr(kv, "_verify_anc", None) is None
    with kv.verifying(tree=[-1, 0, 0, 1]):
        assert kv._verifying and list(kv._verify_anc) == [0b1, 0b11, 0b101, 0b1011]
        with kv.verifying():
            assert kv._verifying and kv._verify_anc is None
        assert list(kv._verify_anc) == [0b1, 0b11, 0b101, 0b1011]
    assert not kv._verifying and kv._verify_anc is None
    with pytest.raises(ops.KvzError, match="ancestor_masks"):
        with kv.verifying(tree=[-1, 1]):
            pass
    assert not kv._verifying and kv._verify_anc is None
