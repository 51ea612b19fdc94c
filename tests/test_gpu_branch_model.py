"""GPU: beam search, n answers to one query and keep-a-branch over one pruned cache (tiny random-init Llama / Qwen2 and the recipe of
tests/test_gpu_fork_model.py) against the sequential path."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-2          # |logit difference| <= BOUND x max|logits|: what the fork tests allow two attention routes of the same math


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


def make(family, max_new_tokens=6):
    from kvzip_amd.wrapper import ModelKVzip
    m = ModelKVzip(tiny_model(family=family), name=f"tiny-{family}", max_new_tokens=max_new_tokens, cache_kwargs=dict(verbose=False))
    g = torch.Generator().manual_seed(1)
    m.set_prompt_ids(torch.randint(0, 160, (1, 5), generator=g), torch.randint(0, 160, (1, 3), generator=g))
    rep = (torch.randint(0, 160, (1, 7), generator=g), torch.randint(0, 160, (1, 9), generator=g))
    ctx = torch.randint(0, 160, (1, 300), generator=g)
    queries = [m.apply_template(torch.randint(0, 160, (1, n), generator=g)) for n in (11, 4, 23)]   # three different lengths
    kv = m.prefill(ctx, prefill_chunk_size=128, do_score=False)
    m.scoring(kv, ctx, chunk_size=100, repeat_prompt_ids=rep)
    kv.prune(0.4)
    return m, kv, queries


class Sequential:
    """Last-position logits of the sequential path for a query followed by a token history: the query as one first step, then one
    token per decode step; the cache is sliced back every time.  Results are kept, so a prefix is never computed twice."""

    def __init__(self, m, kv, q):
        self.m, self.kv, self.q, self.memo, self.max_abs = m, kv, q.to(DEV), {}, 0.0

    def logits(self, hist):
        hist = tuple(int(t) for t in hist)
        if hist not in self.memo:
            seen = self.kv._seen_tokens
            with torch.inference_mode():
                lg = self.m.model(self.q, past_key_values=self.kv, use_cache=True).logits[:, -1]
                self.memo.setdefault((), lg[0].float().cpu())
                for i, t in enumerate(hist):
                    lg = self.m.model(torch.tensor([[t]], device=DEV), past_key_values=self.kv, use_cache=True).logits[:, -1]
                    self.memo.setdefault(hist[:i + 1], lg[0].float().cpu())
            self.kv.slice(seen)
        self.max_abs = max(self.max_abs, float(self.memo[hist].abs().max()))
        return self.memo[hist]

    def logprob(self, toks):
        return sum(float(torch.log_softmax(self.logits(toks[:i]), -1)[toks[i]]) for i in range(len(toks)))


def held_rows(kv):
    out = []
    for l in range(kv.n_layers):
        seg, lens = kv.info["seg_start"][l].tolist(), kv.info["len_k_host"][l]
        out.append([(kv.key_cache[l][seg[h]:seg[h] + lens[h]].clone(), kv.value_cache[l][seg[h]:seg[h] + lens[h]].clone())
                    for h in range(len(lens))])
    return out


def assert_untouched(kv, rows, seen, off):
    assert kv.get_seq_length() == seen and kv._seen_tokens == seen and kv.info["offset"] == off
    now = held_rows(kv)
    for a, b in zip(rows, now):
        for (k0, v0), (k1, v1) in zip(a, b):
            assert torch.equal(k0, k1) and torch.equal(v0, v1)


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_teacher_forced_reorder(family):
    """3 branches, 5 steps, scripted parents - a fan-out of empty tails, a fan-out that drops a branch, a swap, an identity step, a
    fan-out of one slot to all - and scripted tokens: at every step each slot's logits are the sequential path's logits for that
    slot's token history within 1e-2 x max|logits|.  Nothing depends on an argmax."""
    m, kv, queries = make(family)
    q = queries[0].to(DEV)
    seq = Sequential(m, kv, q)
    g = torch.Generator().manual_seed(5)
    # (parents, the slot every hypothesis lives in afterwards, the copies) - written out by hand from the rule: a parent's first child
    # stays in the parent's slot, every further child takes the lowest slot whose occupant has no child
    script = [([0, 0, 0], [0, 1, 2], [(0, 1), (0, 2)]), ([0, 0, 1], [0, 2, 1], [(0, 2)]), ([1, 0, 2], [1, 0, 2], []),
              ([0, 1, 2], [0, 1, 2], []), ([2, 2, 2], [2, 0, 1], [(2, 0), (2, 1)])]
    tokens = torch.randint(0, 160, (len(script), 3), generator=g).tolist()
    # the histories the script produces, slot by slot, and the sequential logits for each (before the fork: slice() ends a fork's base)
    hist, want = [[], [], []], []
    for (parents, slots, _), toks in zip(script, tokens):
        new = [None] * 3
        for i, s in enumerate(slots):
            new[s] = hist[parents[i]] + [toks[i]]
        hist = new
        want.append([seq.logits(h) for h in hist])
    seen, off = kv._seen_tokens, list(kv.info["offset"])
    worst = 0.0
    with torch.inference_mode():
        m.model(q, past_key_values=kv, use_cache=True)                # the query's first step, once, on the base cache
        pos0 = kv.get_seq_length()
        fork = kv.fork(3, tail_capacity=2)                            # (outgrown on the way: the tails are re-allocated between reorders)
        for step, ((parents, slots, pairs), toks) in enumerate(zip(script, tokens)):
            before = [[(fork.tail_k[l][b].clone(), fork.tail_v[l][b].clone()) if step else None for b in range(3)] for l in range(2)]
            assert fork.reorder(parents) == slots
            for l in range(2):                                        # the copied tails, bit for bit (step 0: the tails are empty)
                for s, d in pairs:
                    assert fork.tail_len[l][d] == fork.tail_len[l][s] == step
                    if step:
                        assert torch.equal(fork.tail_k[l][d, :, :step], before[l][s][0][:, :step])
                        assert torch.equal(fork.tail_v[l][d, :, :step], before[l][s][1][:, :step])
            cur = torch.zeros(3, 1, dtype=torch.long, device=DEV)
            for i, s in enumerate(slots):
                cur[s] = toks[i]
            pos = torch.full((3, 1), pos0 + step, dtype=torch.long, device=DEV)
            lg = m.model(cur, past_key_values=fork, use_cache=True, position_ids=pos).logits[:, -1].float().cpu()
            for s in range(3):
                w = want[step][s]
                worst = max(worst, float((lg[s] - w).abs().max() / w.abs().max()))
                assert (lg[s] - w).abs().max() <= BOUND * w.abs().max(), (family, "step", step, "slot", s)
    print(f"\nBRANCH model {family}: worst |logit difference| / max|logits| over {len(script)} steps x 3 slots: {worst:.2e}")
    assert fork.tail_len == [[5, 5, 5], [5, 5, 5]] and fork.active == [True] * 3
    kv.slice(seen)
    assert kv.info["offset"] == [0] * len(off)


def python_beam_search(seq, B, max_new, lp):
    """Plain beam search (no EOS: the tiny models have none) that scores every hypothesis from scratch on the sequential path."""
    beams = [([], 0.0)]
    for _ in range(max_new):
        cands = []
        for toks, s in beams:
            logp = torch.log_softmax(seq.logits(toks), -1)
            for t in torch.topk(logp, B).indices.tolist():
                cands.append((toks + [t], seq.logprob(toks + [t])))
        beams = sorted(cands, key=lambda c: -c[1])[:B]
    return [(s / max_new ** lp, toks) for toks, s in beams]


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_generate_beam(family):
    m, kv, queries = make(family)
    m.gen_kwargs.pop("eos_token_id", None)          # (the reference search below is the plain one: no hypothesis ends early)
    q = queries[0]
    rows, seen, off = held_rows(kv), kv._seen_tokens, list(kv.info["offset"])
    # one beam is greedy decoding (compared the way test_generate_batch compares: an argmax may tie)
    greedy = m.generate(q, kv=kv, return_ids=True)
    one = m.generate_beam(q, kv, num_beams=1, return_ids=True)
    assert one.shape == greedy.shape == (1, 5)
    assert_untouched(kv, rows, seen, off)
    # ... and with an EOS id set it ends where generate ends, at the first EOS, token for token (as test_generate_samples compares),
    # under every length penalty - the runner-up token does not live on past the EOS.  EOS := the third greedy token
    m.gen_kwargs["eos_token_id"] = int(greedy[0, 2])
    short = m.generate(q, kv=kv, return_ids=True)
    print(f"\nBEAM {family}: greedy {greedy[0].tolist()}, EOS {int(greedy[0, 2])}: generate ends after {short.shape[1]} tokens")
    assert short.shape[1] <= 2 and torch.equal(short, greedy[:, :short.shape[1]])
    for lp in (1.0, 0.0, -1.0):
        one = m.generate_beam(q, kv, num_beams=1, length_penalty=lp, return_ids=True)
        assert torch.equal(one, short), (lp, one.tolist(), short.tolist())
        assert len(m.last_beam_hypotheses) == 1 and m.last_beam_hypotheses[0][1] == greedy[0, :short.shape[1] + 1].tolist()
    kept = m.generate_beam(q, kv, num_beams=1, update_cache=True, return_ids=True)      # the EOS-ended answer, kept
    assert torch.equal(kept, short) and kv._seen_tokens == seen + q.shape[1] + short.shape[1]
    kv.slice(seen)
    kv.prefill_ids = kv.prefill_ids[:, :-(q.shape[1] + short.shape[1])]
    assert_untouched(kv, rows, seen, off)
    m.gen_kwargs.pop("eos_token_id")
    assert isinstance(m.generate_beam(q, kv, num_beams=2), str)
    # three beams, four tokens, against the exhaustive re-scoring
    m.gen_kwargs["max_new_tokens"] = 4
    seq = Sequential(m, kv, q)
    ref = python_beam_search(seq, 3, 4, 1.0)
    got = m.generate_beam(q, kv, num_beams=3, return_ids=True)
    assert_untouched(kv, rows, seen, off)
    score, toks = m.last_beam_hypotheses[0]
    assert got.shape == (1, 3) and got[0].tolist() == toks[:-1] and len(toks) == 4
    mine = seq.logprob(toks) / 4 ** 1.0
    # a logit error of e = BOUND x max|logits| moves a log-probability by at most 2e (the logit itself and the log-sum-exp), a sum over
    # 4 tokens by 8e and the score by 8e / 4; the search compares two hypotheses, each mis-scored by that much: 2 x 8e / 4
    e = BOUND * seq.max_abs
    margin = 2 * 4 * 2 * e / 4 ** 1.0
    print(f"\nBEAM {family}: returned {toks} re-scored {mine:.4f} (the search's own score {score:.4f}), exhaustive best {ref[0][1]} "
          f"{ref[0][0]:.4f}, margin {margin:.4f}")
    assert mine >= ref[0][0] - margin
    assert abs(score - mine) <= margin / 2
    three = m.generate_beam(q, kv, num_beams=3, return_ids=True, num_return=3)
    assert len(three) == 3 and torch.equal(three[0], got) and all(x.shape == (1, 3) for x in three)
    assert len(m.last_beam_hypotheses) == 3                             # at the token budget too: the best num_beams, no more
    from kvzip_amd.ops import KvzError
    with pytest.raises(KvzError, match="at most 16 branches"):
        m.generate_beam(q, kv, num_beams=17)
    assert_untouched(kv, rows, seen, off)
    # a cache that cannot be forked (not pruned) is refused before the query's rows are appended to it
    g = torch.Generator().manual_seed(2)
    plain = m.prefill(torch.randint(0, 160, (1, 40), generator=g), do_score=False)
    n = plain._seen_tokens
    for call in (lambda: m.generate_beam(q, plain, num_beams=2), lambda: m.generate_samples(q, plain, 2)):
        with pytest.raises(KvzError, match="needs a pruned"):
            call()
        assert plain._seen_tokens == n and plain.get_seq_length() == n


def test_generate_beam_update_cache():
    """The best beam's rows are committed: the cache is as after a sequential turn with the same tokens."""
    m, kv, queries = make("llama", max_new_tokens=4)
    m2, kv2, _ = make("llama", max_new_tokens=4)
    m.gen_kwargs.pop("eos_token_id", None)
    q, follow = queries[0], queries[1].to(DEV)
    seen, n0 = kv._seen_tokens, kv.prefill_ids.shape[1]
    a = m.generate_beam(q, kv, num_beams=3, update_cache=True, return_ids=True)
    t = q.shape[1] + a.shape[1]
    assert kv._seen_tokens == seen + t and kv.info["offset"] == [t, t] and kv.prefill_ids.shape[1] == n0 + t
    assert torch.equal(kv.prefill_ids[:, n0:], torch.cat([q.to(DEV), a], dim=1))
    m2(torch.cat([q.to(DEV), a], dim=1), kv2, update_cache=True)         # the same turn, sequentially, on a cache of its own
    assert kv2._seen_tokens == kv._seen_tokens and kv2.info["offset"] == kv.info["offset"]
    with torch.inference_mode():
        l1 = m.model(follow, past_key_values=kv, use_cache=True).logits[0, -1].float().cpu()
        l2 = m2.model(follow, past_key_values=kv2, use_cache=True).logits[0, -1].float().cpu()
    assert (l1 - l2).abs().max() <= BOUND * l2.abs().max()
    # a hypothesis that ends in EOS wins (a strongly negative length penalty prefers the shortest): its slot may be gone, so its
    # answer's rows go through the base on the sequential path - same bookkeeping
    kv2.slice(seen)
    kv.slice(seen)
    eos = int(a[0, 1])                               # the best answer's second token: [a0, EOS] ranks among the first beams at step 2
    m2.gen_kwargs["eos_token_id"] = eos
    n2 = kv2.prefill_ids.shape[1]
    b = m2.generate_beam(q, kv2, num_beams=3, length_penalty=-5.0, update_cache=True, return_ids=True)
    score, toks = m2.last_beam_hypotheses[0]
    assert toks[-1] == eos and b[0].tolist() == toks[:-1] and len(toks) <= 2
    assert all(eos not in t[:-1] for _, t in m2.last_beam_hypotheses)
    t2 = q.shape[1] + b.shape[1]
    assert kv2._seen_tokens == seen + t2 and kv2.info["offset"] == [t2, t2] and kv2.prefill_ids.shape[1] == n2 + t2
    assert torch.equal(kv2.prefill_ids[:, n2:], torch.cat([q.to(DEV), b], dim=1))
    m(torch.cat([q.to(DEV), b], dim=1), kv, update_cache=True)           # the same turn, sequentially, on the other cache
    assert kv._seen_tokens == kv2._seen_tokens and kv.info["offset"] == kv2.info["offset"]
    with torch.inference_mode():                                        # the rows and positions are the sequential turn's: a follow-up agrees
        l1 = m2.model(follow, past_key_values=kv2, use_cache=True).logits[0, -1].float().cpu()
        l2 = m.model(follow, past_key_values=kv, use_cache=True).logits[0, -1].float().cpu()
    assert (l1 - l2).abs().max() <= BOUND * l2.abs().max()
    kv2.slice(seen + t2)
    assert isinstance(m2.generate(follow, kv=kv2), str)


def test_generate_batch_keep():
    m, kv, queries = make("llama")
    m2, kv2, _ = make("llama")
    m3, kv3, _ = make("llama")
    rows, seen, n0 = held_rows(kv), kv._seen_tokens, kv.prefill_ids.shape[1]
    forks = []
    fork_of = kv.fork
    kv.fork = lambda *a, **k: forks.append(fork_of(*a, **k)) or forks[-1]
    answers = m.generate_batch(queries, kv, return_ids=True, keep=1)
    del kv.fork
    fork, a = forks[0], answers[1]
    t = queries[1].shape[1] + a.shape[1]
    assert len(forks) == 1 and all(x.shape == (1, 5) for x in answers) and fork.tail_len[0][1] == t
    # the base's new rows are branch 1's tail, bit for bit; the rows it held are as they were
    for l in range(kv.n_layers):
        seg, lens = kv.info["seg_start"][l].tolist(), kv.info["len_k_host"][l]
        for h in range(len(lens)):
            r0 = seg[h] + lens[h]
            assert torch.equal(kv.key_cache[l][r0:r0 + t], fork.tail_k[l][1, h, :t])
            assert torch.equal(kv.value_cache[l][r0:r0 + t], fork.tail_v[l][1, h, :t])
            assert torch.equal(kv.key_cache[l][seg[h]:r0], rows[l][h][0]) and torch.equal(kv.value_cache[l][seg[h]:r0], rows[l][h][1])
    # lengths and prefill_ids as after the sequential multi-turn call
    s = m2.generate(queries[1], kv=kv2, update_cache=True, return_ids=True)
    assert s.shape == a.shape
    assert kv._seen_tokens == kv2._seen_tokens == seen + t and kv.info["offset"] == kv2.info["offset"] == [t, t]
    assert kv.prefill_ids.shape == kv2.prefill_ids.shape and torch.equal(kv.prefill_ids[:, n0:], torch.cat([queries[1].to(DEV), a], dim=1))
    # a follow-up turn: logits within the bound of the follow-up on a cache that took the same turn sequentially (the kept answer's
    # tokens teacher-forced, so that an argmax tie between the two routes cannot make the conversations differ)
    m3(torch.cat([queries[1].to(DEV), a], dim=1), kv3, update_cache=True)
    follow = queries[2].to(DEV)
    with torch.inference_mode():
        l1 = m.model(follow, past_key_values=kv, use_cache=True).logits[0, -1].float().cpu()
        l3 = m3.model(follow, past_key_values=kv3, use_cache=True).logits[0, -1].float().cpu()
    assert (l1 - l3).abs().max() <= BOUND * l3.abs().max()
    kv.slice(seen)
    assert isinstance(m.generate(queries[0], kv=kv), str)               # an ordinary cache again
    # the closed fork
    from kvzip_amd.ops import KvzError
    z = torch.zeros(3, 4, 1, 64, dtype=torch.float16, device=DEV)
    for hook in (lambda: fork.update_attend(z, z[:, :2], z[:, :2], 0), lambda: fork.first_step(z[:1], z[:1, :2], z[:1, :2], 0),
                 lambda: fork.reorder([0, 1, 2]), lambda: fork.commit(1)):
        with pytest.raises(KvzError, match="closed"):
            hook()
    # keep= needs all queries in one wave (G = 2: 16 branches), and a query to keep
    with pytest.raises(KvzError, match="one wave"):
        m.generate_batch(queries * 6, kv, keep=0)
    with pytest.raises(KvzError, match="names none"):
        m.generate_batch(queries, kv, keep=3)


def test_generate_samples():
    m, kv, queries = make("llama")
    m.gen_kwargs.pop("eos_token_id", None)          # (every answer runs to the token budget: the shapes below are fixed)
    q = queries[2]
    rows, seen, off = held_rows(kv), kv._seen_tokens, list(kv.info["offset"])
    greedy = m.generate(q, kv=kv, return_ids=True)
    same = m.generate_samples(q, kv, 3, return_ids=True)
    assert len(same) == 3 and all(x.shape == greedy.shape for x in same)
    assert all(torch.equal(x, greedy) for x in same)                   # do_sample=False: every branch is generate's greedy answer
    assert_untouched(kv, rows, seen, off)
    m.gen_kwargs.update(do_sample=True, temperature=1.5)
    m.sample_generator = torch.Generator(device=DEV).manual_seed(11)
    first = m.generate_samples(q, kv, 5, return_ids=True)
    assert len(first) == 5 and all(x.shape == (1, 5) for x in first)
    assert len({tuple(x[0].tolist()) for x in first}) > 1               # 5 draws of 5 tokens at temperature 1.5 over 160 tokens
    assert_untouched(kv, rows, seen, off)
    m.sample_generator = torch.Generator(device=DEV).manual_seed(11)
    again = m.generate_samples(q, kv, 5, return_ids=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))         # seeded: the same answers
    texts = m.generate_samples(q, kv, 18)                                # more than one wave (G = 2: 16 branches)
    assert len(texts) == 18 and all(isinstance(t, str) for t in texts)
    assert_untouched(kv, rows, seen, off)
