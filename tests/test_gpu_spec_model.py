"""GPU: speculative decoding on a pruned cache through the model (tiny random-init Llama / Qwen2 of tests/test_gpu_fork_model.py's
sizes): teacher-forced verify steps against the sequential path's logits, ModelKVzip.generate_speculative with three drafters against
generate, the cache it leaves, EOS inside an accepted run, what it refuses, and a slack that grows mid-generation.

Token equality is asserted at every position; before that every test asserts that the sequential path's top-2 logit margin exceeds
2e-2 x max|logits| at every compared step (twice the 1e-2 x max|logits| by which two routes of the same math may differ), so that no
position is left out.  MODEL_SEED / QUERY_SEED / FOLLOW_SEED are the seeds of the model's random init and of the queries' generators
for which that holds (found by trying seeds in order, on the sequential path alone)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL_SEED = {"llama": 0, "qwen2": 2}           # torch.manual_seed before the model's random init (0: tests/test_gpu_fork_model's)
QUERY_SEED = {"llama": 1005, "qwen2": 1002}
FOLLOW_SEED = {"llama": 2000, "qwen2": 2002}
STEPS = 42          # 1 + (1 + 1) + (2 + 1) + (3 + 1) + (31 + 1): the query's step, then verify steps with runs of 1, 2, 3 and the cap
M = 12              # max_new_tokens of the generation tests


def tiny_model(family, dtype=torch.float16):
    """tests/test_gpu_fork_model.tiny_model's sizes, with this file's seed of the random init."""
    sizes = dict(vocab_size=160, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                 num_key_value_heads=2, max_position_embeddings=4096)
    if family == "llama":
        from transformers import LlamaConfig, LlamaForCausalLM as Model
        cfg = LlamaConfig(head_dim=64, **sizes)
    else:
        from transformers import Qwen2Config, Qwen2ForCausalLM as Model
        cfg = Qwen2Config(**sizes)
    torch.manual_seed(MODEL_SEED[family])
    return Model(cfg).to(dtype).to(DEV).eval()


def make(family, max_new_tokens=M, **cache_kwargs):
    """tests/test_gpu_fork_model.make with this file's model seed, query and cache settings."""
    from kvzip_amd.wrapper import ModelKVzip
    m = ModelKVzip(tiny_model(family), name=f"tiny-{family}", max_new_tokens=max_new_tokens,
                   cache_kwargs=dict(verbose=False, **cache_kwargs))
    g = torch.Generator().manual_seed(1)
    m.gen_kwargs.pop("eos_token_id", None)      # (the configs' default EOS is an ordinary token of these random models)
    m.set_prompt_ids(torch.randint(0, 160, (1, 5), generator=g), torch.randint(0, 160, (1, 3), generator=g))
    rep = (torch.randint(0, 160, (1, 7), generator=g), torch.randint(0, 160, (1, 9), generator=g))
    ctx = torch.randint(0, 160, (1, 300), generator=g)
    kv = m.prefill(ctx, prefill_chunk_size=128, do_score=False)
    m.scoring(kv, ctx, chunk_size=100, repeat_prompt_ids=rep)
    kv.prune(0.4)
    return m, kv, ctx, rep


def query(m, seed):
    return m.apply_template(torch.randint(0, 160, (1, 9), generator=torch.Generator().manual_seed(seed)))


def sequential(m, kv, q, steps):
    """The sequential path's tokens (python ints) and logits (as tests/test_gpu_fork_model._sequential_logits; the cache is put back
    afterwards), after asserting the top-2 margin at every step."""
    seen = kv._seen_tokens
    cur, toks, logits = q, [], []
    with torch.inference_mode():
        for _ in range(steps):
            out = m.model(cur, past_key_values=kv, use_cache=True).logits[:, -1]
            logits.append(out[0].float().cpu())
            cur = out.argmax(-1, keepdim=True)
            toks.append(cur)
    kv.rewind(kv._seen_tokens - seen)       # (not slice: rows an earlier turn appended stay)
    lg = torch.stack(logits)
    top = lg.topk(2, -1).values
    rel = (top[:, 0] - top[:, 1]) / lg.abs().amax(-1)
    print(f"\nSPEC model: smallest top-2 margin / max|logits| over {steps} sequential steps: {float(rel.min()):.3e}")
    assert bool((rel > 2e-2).all()), ("top-2 margin below 2e-2 x max|logits| at steps", (rel <= 2e-2).nonzero().flatten().tolist())
    return [int(t) for t in toks], logits


def cache_state(kv):
    lens, seg = kv.info["len_k_host"], [s.tolist() for s in kv.info["seg_start"]]
    rows = [torch.cat([kv.key_cache[l][seg[l][h]:seg[l][h] + lens[l][h] + kv.info["offset"][l]] for h in range(len(lens[l]))] +
                      [kv.value_cache[l][seg[l][h]:seg[l][h] + lens[l][h] + kv.info["offset"][l]] for h in range(len(lens[l]))]).clone()
            for l in range(len(lens))]
    return kv._seen_tokens, list(kv.info["offset"]), rows


def same_state(a, b):
    return a[0] == b[0] and a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_teacher_forced_verify_steps_match_the_sequential_path(family):
    """Verify steps fed the sequential path's own tokens, in runs of 1, 2, 3 and the cap (64 // G - 1 = 31): every position's logits
    within 1e-2 x max|logits| of the sequential path's (the bound test_gpu_fork_model uses for two routes of the same math), and the
    whole draft accepted."""
    from kvzip_amd.draft import accept_greedy
    m, kv, _, _ = make(family, max_new_tokens=STEPS)
    q = query(m, QUERY_SEED[family])
    toks, logits = sequential(m, kv, q, STEPS)
    cap = m._draft_len(10 ** 6)
    assert cap == 31
    before = cache_state(kv)
    calls = []
    real = kv.verify_attend
    kv.verify_attend = lambda *a, **k: (calls.append(a[0].shape[-2]), real(*a, **k))[1]
    worst = 0.0
    ids = torch.tensor(toks, dtype=torch.long, device=DEV)
    with torch.inference_mode():
        lg = m.model(q, past_key_values=kv, use_cache=True).logits[0, -1].float().cpu()
        assert (lg - logits[0]).abs().max() <= 1e-2 * logits[0].abs().max()
        j = 0       # index of the token the next step starts from
        for d in (1, 2, 3, cap):
            pos = torch.arange(kv._seen_tokens, kv._seen_tokens + d + 1, device=DEV)[None]
            with kv.verifying():
                lg = m.model(ids[None, j:j + d + 1], past_key_values=kv, use_cache=True, position_ids=pos).logits[0].float().cpu()
            for i in range(d + 1):
                want = logits[j + 1 + i]
                worst = max(worst, float((lg[i] - want).abs().max() / want.abs().max()))
                assert (lg[i] - want).abs().max() <= 1e-2 * want.abs().max(), (family, "run", d, "position", i)
            am = lg.argmax(-1)
            assert accept_greedy(ids[j + 1:j + d + 1].cpu(), am) == d and int(am[d]) == toks[j + d + 1], (family, "run", d)
            j += d + 1
    print(f"\nSPEC model {family}: worst |logit difference| / max|logits| over {j} verified positions: {worst:.2e}")
    L = len(kv.info["offset"])
    assert calls == [t for d in (1, 2, 3, cap) for t in [d + 1] * L], "every run took the verify path, once per layer"
    assert kv.info["offset"] == [q.shape[1] + j] * L and kv._seen_tokens == before[0] + q.shape[1] + j
    kv.rewind(j)
    kv.rewind(q.shape[1])
    assert same_state(cache_state(kv), before)


def _drafters(full, base_len):
    def k_of(history):
        return history.shape[0] - base_len              # answer tokens in the history so far

    def right(history, n):
        k = k_of(history)
        return torch.tensor(full[k:k + n], dtype=torch.long)

    def wrong(history, n):
        return (right(history, n) + 1) % 160

    def two_right(history, n):
        d = right(history, n)
        d[2:] = (d[2:] + 1) % 160
        return d
    return right, wrong, two_right


def _expected_stats(max_new, nd, n_right):
    out, st = 1, {"steps": 0, "tokens": 0, "drafted": 0, "accepted": 0}
    while out < max_new:
        d = min(nd, max_new - out - 1)
        a = min(d, n_right)
        st["steps"] += 1; st["drafted"] += d; st["accepted"] += a; st["tokens"] += a + 1
        out += a + 1
    return st


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_generate_speculative_with_three_drafters(family):
    m, kv, _, _ = make(family)
    q = query(m, QUERY_SEED[family])
    full, _ = sequential(m, kv, q, M)
    before = cache_state(kv)
    ref = m.generate(q, kv=kv, return_ids=True)
    assert ref[0].tolist() == full[:-1] and same_state(cache_state(kv), before)
    base_len = kv.prefill_ids.shape[1] + q.shape[1]
    right, wrong, two_right = _drafters(full, base_len)
    rewinds = []
    real = kv.rewind
    kv.rewind = lambda n: (rewinds.append(n), real(n))[1]
    nd = 3
    for name, drafter, n_right in (("right", right, nd), ("wrong", wrong, 0), ("two right", two_right, 2)):
        del rewinds[:]
        ids, stats = m.generate_speculative(q, kv, draft=drafter, num_draft=nd, return_ids=True, return_stats=True)
        print(f"\nSPEC model {family} drafter '{name}': {stats}")
        assert ids[0].tolist() == ref[0].tolist(), (family, name)
        assert stats == _expected_stats(M, nd, n_right), (family, name)
        assert same_state(cache_state(kv), before), (family, name, "update_cache=False leaves the cache as it was")
        if name == "right":
            assert stats["accepted"] == stats["drafted"] > 0 and not any(rewinds)
        if name == "wrong":
            assert stats["accepted"] == 0 and stats["tokens"] == stats["steps"]
            drafted_steps = [min(nd, M - 1 - i - 1) for i in range(M - 1)]
            assert [n for n in rewinds if n] == [d for d in drafted_steps if d], "every step of the wrong drafter rewinds its draft"
    # the default drafter (prompt lookup over prefill ++ query ++ answer) and the default draft length give generate's ids as well
    ids, stats = m.generate_speculative(q, kv, return_ids=True, return_stats=True)
    assert ids[0].tolist() == ref[0].tolist() and stats["tokens"] == M - 1 and same_state(cache_state(kv), before)
    assert isinstance(m.generate_speculative(q, kv), str)


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_update_cache_leaves_what_generate_leaves(family):
    ma, kva, _, _ = make(family)
    mb, kvb, _, _ = make(family)
    q = query(ma, QUERY_SEED[family])
    full, _ = sequential(ma, kva, q, M)
    right = _drafters(full, kva.prefill_ids.shape[1] + q.shape[1])[0]
    a = ma.generate(q, kv=kva, update_cache=True, return_ids=True)
    b = mb.generate_speculative(q, kvb, draft=right, num_draft=3, update_cache=True, return_ids=True)
    assert torch.equal(a, b)
    assert kva._seen_tokens == kvb._seen_tokens and kva.info["offset"] == kvb.info["offset"] == [q.shape[1] + M - 1] * 2
    assert torch.equal(kva.prefill_ids, kvb.prefill_ids)
    # the next turn on both caches
    q2 = query(ma, FOLLOW_SEED[family])
    ma.gen_kwargs["max_new_tokens"] = mb.gen_kwargs["max_new_tokens"] = 5
    sequential(ma, kva, q2, 5)
    assert torch.equal(ma.generate(q2, kv=kva, return_ids=True), mb.generate(q2, kv=kvb, return_ids=True))


def test_eos_inside_an_accepted_run_ends_the_answer_there():
    m, kv, _, _ = make("llama")
    q = query(m, QUERY_SEED["llama"])
    full, _ = sequential(m, kv, q, M)
    right = _drafters(full, kv.prefill_ids.shape[1] + q.shape[1])[0]
    nd = 3
    # an answer position inside an accepted run (steps produce positions 1-4, 5-8, ...: the last of each is the model's own token)
    # whose token did not occur before it
    js = [j for j in range(1, M - 1) if j % (nd + 1) != 0 and full[j] not in full[:j]]
    assert js, full
    j = js[0]
    m.gen_kwargs["eos_token_id"] = full[j]
    before = cache_state(kv)
    ref = m.generate(q, kv=kv, return_ids=True)
    assert ref[0].tolist() == full[:j]
    ids, stats = m.generate_speculative(q, kv, draft=right, num_draft=nd, return_ids=True, return_stats=True)
    assert ids[0].tolist() == full[:j] and same_state(cache_state(kv), before)
    assert stats["tokens"] == j          # the EOS is the last token produced: nothing behind it counts
    m.generate_speculative(q, kv, draft=right, num_draft=nd, update_cache=True)
    assert kv._seen_tokens == before[0] + q.shape[1] + j and kv.info["offset"] == [q.shape[1] + j] * 2
    assert kv.prefill_ids.shape[1] == 305 + q.shape[1] + j


def test_what_generate_speculative_refuses():
    m, kv, ctx, rep = make("llama")
    q = query(m, QUERY_SEED["llama"])
    m.gen_kwargs["do_sample"] = True
    with pytest.raises(ValueError, match="greedy"):
        m.generate_speculative(q, kv)
    m.gen_kwargs["do_sample"] = False
    dense = m.prefill(ctx, prefill_chunk_size=128, do_score=False)
    with pytest.raises(ValueError, match="use generate"):
        m.generate_speculative(q, dense)
    m.cache_kwargs["layout"] = "packed"
    packed = m.prefill(ctx, prefill_chunk_size=128, do_score=False)
    m.scoring(packed, ctx, chunk_size=100, repeat_prompt_ids=rep)
    packed.prune(0.4)
    with pytest.raises(ValueError, match="use generate"):
        m.generate_speculative(q, packed)
    from kvzip_amd.ops import KvzError
    with pytest.raises(KvzError, match="rewind"):
        kv.rewind(1)                     # nothing was appended since the prune


def test_slack_grows_mid_generation():
    """slack = 16: the 12 query tokens fit, the answer outgrows it inside a verify step; same answer as with room to spare."""
    m0, kv0, _, _ = make("llama")
    q = query(m0, QUERY_SEED["llama"])
    full, _ = sequential(m0, kv0, q, M)
    m, kv, _, _ = make("llama", slack=16)
    right = _drafters(full, kv.prefill_ids.shape[1] + q.shape[1])[0]
    assert kv.slack == 16 and q.shape[1] == 12
    grown = []
    real = kv._grow_slack
    kv._grow_slack = lambda need: (grown.append((need, getattr(kv, "_verifying", False))), real(need))[1]
    ids = m.generate_speculative(q, kv, draft=right, num_draft=3, update_cache=True, return_ids=True)
    assert ids[0].tolist() == full[:-1]
    assert kv.slack > 16 and grown and grown[0][1], "the slack grew inside a verify step"
    assert kv.info["offset"] == [q.shape[1] + M - 1] * 2
