"""GPU: ModelKVzip.generate_multi - one query per cache, several independent pruned caches decoded together (tiny random-init Llama /
Qwen2 of tests/test_gpu_fork_model.py's sizes) against the sequential generate on clones of the caches."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTX = (300, 171)        # two different contexts: the caches differ in every length


def tiny_model(dtype=torch.float16, family="llama"):
    if family == "llama":
        from transformers import LlamaConfig, LlamaForCausalLM as M
        cfg = LlamaConfig(vocab_size=160, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                          num_attention_heads=4, num_key_value_heads=2, head_dim=64, max_position_embeddings=4096)
    else:
        from transformers import Qwen2Config, Qwen2ForCausalLM as M
        cfg = Qwen2Config(vocab_size=160, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                          num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=4096)
    torch.manual_seed(0)
    return M(cfg).to(dtype).to(DEV).eval()


def make(family, max_new_tokens=6, seed=1):
    """(model, two pruned caches over different contexts, clones of the two - prefilled, scored and pruned the same way -, two queries)"""
    from kvzip_amd.wrapper import ModelKVzip
    m = ModelKVzip(tiny_model(family=family), name=f"tiny-{family}", max_new_tokens=max_new_tokens, cache_kwargs=dict(verbose=False))
    g = torch.Generator().manual_seed(seed)
    m.set_prompt_ids(torch.randint(0, 160, (1, 5), generator=g), torch.randint(0, 160, (1, 3), generator=g))
    rep = (torch.randint(0, 160, (1, 7), generator=g), torch.randint(0, 160, (1, 9), generator=g))
    ctxs = [torch.randint(0, 160, (1, n), generator=g) for n in CTX]
    queries = [m.apply_template(torch.randint(0, 160, (1, n), generator=g)) for n in (11, 4)]

    def caches():
        out = []
        for ctx, ratio in zip(ctxs, (0.4, 0.6)):
            kv = m.prefill(ctx, prefill_chunk_size=128, do_score=False)
            m.scoring(kv, ctx, chunk_size=100, repeat_prompt_ids=rep)
            kv.prune(ratio)
            out.append(kv)
        return out
    kvs, clones = caches(), caches()
    for a, b in zip(kvs, clones):
        assert a.info["len_k_host"] == b.info["len_k_host"]
    return m, kvs, clones, queries


def _sequential_logits(m, kv, q_ids, n_steps):
    """The sequential path's tokens and its last-position logits at every step (greedy), the cache sliced back afterwards."""
    seen = kv._seen_tokens
    cur, toks, logits = q_ids, [], []
    with torch.inference_mode():
        for _ in range(n_steps):
            lg = m.model(cur, past_key_values=kv, use_cache=True).logits[:, -1]
            logits.append(lg[0].float().cpu())
            cur = lg.argmax(-1, keepdim=True)
            toks.append(cur)
    kv.slice(seen)
    return toks, logits


def _teacher_forced(m, kvs, clones, queries, steps):
    """Worst |logit difference| / max|logits| of the batched steps, fed the tokens the sequential path produced on the clones; asserts
    the bound test_gpu_fork_model.py uses for fork versus single decode (1e-2 x max|logits|).  The caches are sliced back."""
    from kvzip_amd.kvcache import CacheBatch
    seq = [_sequential_logits(m, c, q, steps) for c, q in zip(clones, queries)]
    seen = [kv._seen_tokens for kv in kvs]
    batch = CacheBatch(kvs)
    worst = 0.0
    with torch.inference_mode():
        pos = torch.zeros(len(kvs), 1, dtype=torch.long, device=DEV)
        for b, q in enumerate(queries):       # first steps: each cache's own path (bit-identical to the clone's)
            lg = m.model(q.to(DEV), past_key_values=kvs[b], use_cache=True).logits[0, -1].float().cpu()
            assert torch.equal(lg, seq[b][1][0])
            pos[b] = kvs[b].get_seq_length()
        for t in range(1, steps):
            cur = torch.cat([seq[b][0][t - 1] for b in range(len(kvs))], dim=0)      # teacher forcing: the sequential tokens
            lg = m.model(cur, past_key_values=batch, use_cache=True, position_ids=pos).logits[:, -1].float().cpu()
            pos += 1
            for b in range(len(kvs)):
                want = seq[b][1][t]
                worst = max(worst, float((lg[b] - want).abs().max() / want.abs().max()))
                assert (lg[b] - want).abs().max() <= 1e-2 * want.abs().max(), ("step", t, "cache", b)
    for kv, q, s in zip(kvs, queries, seen):
        assert kv.info["offset"] == [q.shape[1] + steps - 1] * 2 and kv._seen_tokens == s + q.shape[1] + steps - 1
        kv.slice(s)
    return worst


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_teacher_forced_logits_match_the_sequential_path(family):
    m, kvs, clones, queries = make(family)
    worst = _teacher_forced(m, kvs, clones, queries, 5)
    print(f"\nMULTI model {family}: worst |logit difference| / max|logits| over 5 steps x 2 caches: {worst:.2e}")


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_generate_multi_matches_generate_on_clones(family):
    """Token ids of generate_multi against two separate generate calls on the clones.  The two attention routes sum in another order,
    so an argmax between two nearly equal logits may tie-break differently: where a sequence's ids differ, the teacher-forced logits
    (the test above, on these very caches) must agree instead; the seed and the contexts of make() are such that the plain comparison
    holds for at least one of the two sequences - asserted."""
    m, kvs, clones, queries = make(family)
    seen = [kv.get_seq_length() for kv in kvs]
    single = [m.generate(q, kv=c, return_ids=True) for q, c in zip(queries, clones)]
    multi = m.generate_multi(queries, kvs, return_ids=True)
    assert len(multi) == 2 and all(a.shape == b.shape == (1, 5) for a, b in zip(single, multi))    # max_new_tokens = 6, the last dropped
    same = [torch.equal(a, b) for a, b in zip(single, multi)]
    print(f"\nMULTI generate {family}: identical token ids per sequence: {same}")
    assert any(same)
    if not all(same):
        _teacher_forced(m, kvs, clones, queries, 5)
    # every cache is as it was, and an ordinary EvictCache again
    for kv, c, s in zip(kvs, clones, seen):
        assert kv.get_seq_length() == s == c.get_seq_length() and kv.info["offset"] == [0, 0]
    again = [m.generate(q, kv=kv, return_ids=True) for q, kv in zip(queries, kvs)]
    assert all(torch.equal(a, b) for a, b in zip(single, again))
    texts = m.generate_multi(queries, kvs)
    assert len(texts) == 2 and all(isinstance(t, str) for t in texts)
    with pytest.raises(ValueError, match="one query per cache"):
        m.generate_multi(queries, kvs[:1])
    # more caches than one wave takes: waves of two, and a last wave of one (the sequential path)
    m.multi_max_caches = 2
    three = m.generate_multi(queries + queries[:1], kvs + clones[:1], return_ids=True)
    assert len(three) == 3 and torch.equal(three[2], single[0]) and [torch.equal(a, b) for a, b in zip(three, multi)] == [True, True]


def test_a_sequence_that_meets_eos_retires_while_the_other_goes_on():
    m, kvs, clones, queries = make("llama", max_new_tokens=8)
    ref = m.generate_multi(queries, kvs, return_ids=True)
    assert all(x.shape[1] == 7 for x in ref)
    ids = [r[0].tolist() for r in ref]
    # EOS := a token one sequence emits and the other emits later or never: the first stops there, the other at its own first
    # occurrence of the token or at the budget (the EOS itself is the dropped last token)
    stop = lambda x, e: x.index(e) if e in x else len(x)  # noqa: E731
    eos = max(set(ids[0]) | set(ids[1]), key=lambda e: abs(stop(ids[1], e) - stop(ids[0], e)))
    m.gen_kwargs["eos_token_id"] = eos
    out = m.generate_multi(queries, kvs, return_ids=True)
    want = [x[:stop(x, eos)] for x in ids]
    print(f"\nMULTI eos {eos}: answer lengths {[len(w) for w in want]} of {[len(x) for x in ids]}")
    assert [o[0].tolist() for o in out] == want
    assert len(want[0]) != len(want[1]) and min(len(w) for w in want) < 7
    assert [kv.get_seq_length() for kv in kvs] == [5 + n for n in CTX] and all(kv.info["offset"] == [0, 0] for kv in kvs)


def test_update_cache_keeps_the_turn():
    """update_cache=True: both caches hold the query and the answer afterwards (rows, offsets, prefill_ids) as the clones do after
    their own generate(update_cache=True), and a following single generate on each gives the clones' tokens."""
    m, kvs, clones, queries = make("qwen2")
    single = [m.generate(q, kv=c, update_cache=True, return_ids=True) for q, c in zip(queries, clones)]
    multi = m.generate_multi(queries, kvs, update_cache=True, return_ids=True)
    g = torch.Generator().manual_seed(5)
    follow = [m.apply_template(torch.randint(0, 160, (1, n), generator=g)) for n in (6, 9)]
    turn_same = [torch.equal(a, b) for a, b in zip(multi, single)]
    for i, (kv, c, a, q) in enumerate(zip(kvs, clones, multi, queries)):
        assert kv.info["offset"] == c.info["offset"] == [q.shape[1] + 5] * 2 and kv.get_seq_length() == c.get_seq_length()
        assert kv.prefill_ids.shape == c.prefill_ids.shape and torch.equal(kv.prefill_ids[:, -5:], a)
    # (update_cache=True again: slice() of the slack layout drops every appended row, the turn before included)
    nxt_multi = [m.generate(f, kv=kv, update_cache=True, return_ids=True) for f, kv in zip(follow, kvs)]
    nxt_single = [m.generate(f, kv=c, update_cache=True, return_ids=True) for f, c in zip(follow, clones)]
    same = [torch.equal(a, b) for a, b in zip(nxt_multi, nxt_single)]
    print(f"\nMULTI update_cache: turn identical {turn_same}, next turn identical {same}")
    assert any(turn_same)
    for i in range(2):      # (a turn whose ids differ by an argmax tie left another history in the cache: nothing to compare)
        if turn_same[i]:
            assert same[i], i
