"""GPU: tree speculative decoding on a pruned cache through the model (the tiny random-init Llama / Qwen2 of tests/test_gpu_spec_model.py,
with its seeds and its top-2 margin check): teacher-forced tree steps - the true continuation as one root-to-leaf path among wrong
siblings - against the sequential path's logits with keep_path between them, ModelKVzip.generate_speculative(tree=True) with four
drafters against generate, the cache it leaves, EOS inside a path, a slack that grows mid-generation, and what it refuses."""
import pytest
import torch

from test_gpu_spec_model import DEV, FOLLOW_SEED, M, QUERY_SEED, cache_state, make, query, same_state, sequential

pytestmark = pytest.mark.gpu
LEVELS = (1, 2, 3, 15)      # verify steps of 3, 5, 7 and 31 nodes: two siblings per level, the right one second
STEPS = 1 + sum(d + 1 for d in LEVELS) + 1      # the query's step, the tree steps (d accepted + the model's own token), a decode step


def two_siblings(right):
    """ids / parents of the nodes behind the root for the true continuation ``right``: per level (wrong, right), both children of the
    previous level's right node; the wrong one is a leaf.  Depth-first order: w1 r1 w2 r2 ...; the true path is nodes 0, 2, 4, ..."""
    ids, parents = [], []
    for lvl, tok in enumerate(right):
        ids += [(tok + 1) % 160, tok]
        parents += [2 * lvl, 2 * lvl]
    return ids, parents


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_teacher_forced_tree_steps_match_the_sequential_path(family):
    """Tree steps fed the sequential path's own tokens as the second sibling of every level: the logits at every node of the true path
    within 1e-2 x max|logits| of the sequential path's (the bound of test_gpu_spec_model), the whole path accepted, and - since every
    later step attends to the rows keep_path moved - the kept rows are the right ones."""
    from kvzip_amd.draft import accept_tree_greedy
    m, kv, _, _ = make(family, max_new_tokens=STEPS)
    q = query(m, QUERY_SEED[family])
    toks, logits = sequential(m, kv, q, STEPS)
    before = cache_state(kv)
    calls = []
    real = kv.verify_attend
    kv.verify_attend = lambda *a, **k: (calls.append(a[0].shape[-2]), real(*a, **k))[1]
    worst = 0.0
    with torch.inference_mode():
        lg = m.model(q, past_key_values=kv, use_cache=True).logits[0, -1].float().cpu()
        assert (lg - logits[0]).abs().max() <= 1e-2 * logits[0].abs().max()
        j = 0       # index of the token the next step starts from
        for d in LEVELS:
            ids, parents = two_siblings(toks[j + 1:j + d + 1])
            t = 2 * d + 1
            depth = [0] + [lvl + 1 for lvl in range(d) for _ in range(2)]
            cur = torch.tensor([[toks[j]] + ids], dtype=torch.long, device=DEV)
            pos = (kv._seen_tokens + torch.tensor(depth, device=DEV))[None]
            seen = kv._seen_tokens
            with kv.verifying(tree=[-1] + parents):
                lg = m.model(cur, past_key_values=kv, use_cache=True, position_ids=pos).logits[0].float().cpu()
            assert kv._seen_tokens == seen + t and kv.info["offset"] == [q.shape[1] + j + t] * 2
            path = [0] + [2 * i + 2 for i in range(d)]
            for i, node in enumerate(path):
                want = logits[j + 1 + i]
                worst = max(worst, float((lg[node] - want).abs().max() / want.abs().max()))
                assert (lg[node] - want).abs().max() <= 1e-2 * want.abs().max(), (family, "levels", d, "node", node)
            am = lg.argmax(-1)
            assert accept_tree_greedy(torch.tensor(ids), parents, am) == path and int(am[path[-1]]) == toks[j + d + 1], (family, d)
            kv.keep_path(path, t)
            assert kv._seen_tokens == seen + d + 1 and kv.info["offset"] == [q.shape[1] + j + d + 1] * 2
            j += d + 1
        # one plain decode step over everything the paths left behind
        lg = m.model(torch.tensor([[toks[j]]], device=DEV), past_key_values=kv, use_cache=True).logits[0, -1].float().cpu()
        assert (lg - logits[j + 1]).abs().max() <= 1e-2 * logits[j + 1].abs().max()
        j += 1
    print(f"\nTREE model {family}: worst |logit difference| / max|logits| over the true paths of {len(LEVELS)} tree steps: {worst:.2e}")
    L = len(kv.info["offset"])
    assert calls == [t for d in LEVELS for t in [2 * d + 1] * L], "every tree step took the verify path, once per layer"
    kv.rewind(j)
    kv.rewind(q.shape[1])
    assert same_state(cache_state(kv), before)


def _drafters(full, base_len):
    def right(history, n):
        k = history.shape[0] - base_len                 # answer tokens in the history so far
        return full[k:k + n]

    def second(history, n):
        ids, parents = two_siblings(right(history, n // 2))
        return torch.tensor(ids, dtype=torch.long), parents

    def wrong_star(history, n):
        return torch.tensor([(x + 1) % 160 for x in right(history, 1)] * n, dtype=torch.long)[:n], [0] * n

    def first_chain(history, n):                        # what a chain drafter makes of `second`'s proposals: the first child
        return torch.tensor([(x + 1) % 160 for x in right(history, 1)], dtype=torch.long)[:n]
    return second, wrong_star, first_chain


def _expected_stats(max_new, nd):
    out, st = 1, {"steps": 0, "tokens": 0, "drafted": 0, "accepted": 0, "nodes": 0}
    while out < max_new:
        lv = min(nd, max_new - out - 1) // 2
        st["steps"] += 1; st["drafted"] += 2 * lv; st["accepted"] += lv; st["tokens"] += lv + 1
        st["nodes"] += 2 * lv + 1 if lv else 0
        out += lv + 1
    return st


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_generate_speculative_tree_with_its_drafters(family):
    m, kv, _, _ = make(family)
    q = query(m, QUERY_SEED[family])
    full, _ = sequential(m, kv, q, M)
    before = cache_state(kv)
    ref = m.generate(q, kv=kv, return_ids=True)
    assert ref[0].tolist() == full[:-1] and same_state(cache_state(kv), before)
    second, wrong_star, first_chain = _drafters(full, kv.prefill_ids.shape[1] + q.shape[1])
    kept = []
    real = kv.keep_path
    kv.keep_path = lambda path, t: (kept.append((list(path), t)), real(path, t))[1]
    nd = 6
    ids, stats = m.generate_speculative(q, kv, draft=second, num_draft=nd, return_ids=True, return_stats=True, tree=True)
    print(f"\nTREE model {family} drafter 'right token second': {stats}")
    assert ids[0].tolist() == ref[0].tolist()
    assert stats == _expected_stats(M, nd)
    assert same_state(cache_state(kv), before), "update_cache=False leaves the cache as it was"
    assert all(path == [0] + [2 * i + 2 for i in range((t - 1) // 2)] for path, t in kept) and kept
    ids, chain = m.generate_speculative(q, kv, draft=first_chain, num_draft=nd, return_ids=True, return_stats=True)
    assert ids[0].tolist() == ref[0].tolist() and chain["accepted"] == 0 and chain["steps"] == M - 1
    assert stats["steps"] < chain["steps"], "the tree form needs fewer forward passes than the chain form on the same proposals"
    del kept[:]
    ids, stats = m.generate_speculative(q, kv, draft=wrong_star, num_draft=nd, return_ids=True, return_stats=True, tree=True)
    assert ids[0].tolist() == ref[0].tolist() and same_state(cache_state(kv), before)
    assert stats["accepted"] == 0 and stats["tokens"] == stats["steps"] == M - 1, "every step of the wrong drafter yields one token"
    assert all(path == [0] for path, _ in kept)
    # the default drafter (lookup_tree over prefill ++ query ++ answer) and the default node budget give generate's ids as well
    ids, stats = m.generate_speculative(q, kv, return_ids=True, return_stats=True, tree=True)
    assert ids[0].tolist() == ref[0].tolist() and stats["tokens"] == M - 1 and same_state(cache_state(kv), before)
    assert isinstance(m.generate_speculative(q, kv, tree=True), str)


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_update_cache_leaves_what_generate_leaves(family):
    ma, kva, _, _ = make(family)
    mb, kvb, _, _ = make(family)
    q = query(ma, QUERY_SEED[family])
    full, _ = sequential(ma, kva, q, M)
    second = _drafters(full, kva.prefill_ids.shape[1] + q.shape[1])[0]
    a = ma.generate(q, kv=kva, update_cache=True, return_ids=True)
    b = mb.generate_speculative(q, kvb, draft=second, num_draft=6, update_cache=True, return_ids=True, tree=True)
    assert torch.equal(a, b)
    assert kva._seen_tokens == kvb._seen_tokens and kva.info["offset"] == kvb.info["offset"] == [q.shape[1] + M - 1] * 2
    assert torch.equal(kva.prefill_ids, kvb.prefill_ids)
    # the next turn on both caches: it attends to the rows the paths left
    q2 = query(ma, FOLLOW_SEED[family])
    ma.gen_kwargs["max_new_tokens"] = mb.gen_kwargs["max_new_tokens"] = 5
    sequential(ma, kva, q2, 5)
    assert torch.equal(ma.generate(q2, kv=kva, return_ids=True), mb.generate(q2, kv=kvb, return_ids=True))


def test_eos_inside_a_path_ends_the_answer_there():
    m, kv, _, _ = make("llama")
    q = query(m, QUERY_SEED["llama"])
    full, _ = sequential(m, kv, q, M)
    second = _drafters(full, kv.prefill_ids.shape[1] + q.shape[1])[0]
    nd, lv = 6, 3
    # an answer position inside an accepted path (steps produce positions 1-4, 5-8, ...: the last of each is the model's own token)
    # whose token did not occur before it
    js = [j for j in range(1, M - 1) if j % (lv + 1) != 0 and full[j] not in full[:j]]
    assert js, full
    j = js[0]
    m.gen_kwargs["eos_token_id"] = full[j]
    before = cache_state(kv)
    ref = m.generate(q, kv=kv, return_ids=True)
    assert ref[0].tolist() == full[:j]
    ids, stats = m.generate_speculative(q, kv, draft=second, num_draft=nd, return_ids=True, return_stats=True, tree=True)
    assert ids[0].tolist() == full[:j] and same_state(cache_state(kv), before)
    assert stats["tokens"] == j          # the EOS is the last token produced: nothing behind it counts
    m.generate_speculative(q, kv, draft=second, num_draft=nd, update_cache=True, tree=True)
    assert kv._seen_tokens == before[0] + q.shape[1] + j and kv.info["offset"] == [q.shape[1] + j] * 2
    assert kv.prefill_ids.shape[1] == 305 + q.shape[1] + j


def test_what_the_tree_form_refuses():
    from kvzip_amd.ops import KvzError
    m, kv, ctx, rep = make("llama")
    q = query(m, QUERY_SEED["llama"])
    m.gen_kwargs["do_sample"] = True
    with pytest.raises(ValueError, match="greedy"):
        m.generate_speculative(q, kv, tree=True)
    m.gen_kwargs["do_sample"] = False
    dense = m.prefill(ctx, prefill_chunk_size=128, do_score=False)
    with pytest.raises(ValueError, match="use generate"):
        m.generate_speculative(q, dense, tree=True)
    with pytest.raises(KvzError, match="keep_path"):
        dense.keep_path([0, 2], 3)
    before = cache_state(kv)
    with pytest.raises(KvzError, match="keep_path"):
        kv.keep_path([0, 2], 3)          # nothing was appended since the prune
    with pytest.raises(KvzError, match="nodes"):     # a forward whose length is not the tree's
        with kv.verifying(tree=[-1, 0, 0]):
            m.model(q[:, :2], past_key_values=kv, use_cache=True)
    assert same_state(cache_state(kv), before), "a refusal touches nothing"


def test_slack_grows_mid_generation():
    """slack = 16: the 12 query tokens fit, the answer outgrows it inside a tree verify step; same answer as with room to spare."""
    m0, kv0, _, _ = make("llama")
    q = query(m0, QUERY_SEED["llama"])
    full, _ = sequential(m0, kv0, q, M)
    m, kv, _, _ = make("llama", slack=16)
    second = _drafters(full, kv.prefill_ids.shape[1] + q.shape[1])[0]
    assert kv.slack == 16 and q.shape[1] == 12
    grown = []
    real = kv._grow_slack
    kv._grow_slack = lambda need: (grown.append((need, getattr(kv, "_verify_anc", None) is not None)), real(need))[1]
    ids = m.generate_speculative(q, kv, draft=second, num_draft=6, update_cache=True, return_ids=True, tree=True)
    assert ids[0].tolist() == full[:-1]
    assert kv.slack > 16 and grown and grown[0][1], "the slack grew inside a tree verify step"
    assert kv.info["offset"] == [q.shape[1] + M - 1] * 2
