"""GPU: ModelKVzip.generate_batch - several queries decoded together over one pruned cache (tiny random-init Llama / Qwen2 of
tests/test_gpu_model.py's sizes) against the sequential generate."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_teacher_forced_logits_match_the_sequential_path(family):
    """Every step of every branch, fed the token ids the sequential path produced, gives the sequential path's logits within
    1e-2 x max|logits| (the bound test_evict_and_retain_generate_the_same uses for two attention routes of the same math)."""
    m, kv, queries = make(family)
    steps = 5
    seq = [_sequential_logits(m, kv, q, steps) for q in queries]
    base_len = kv.get_seq_length()
    fork = kv.fork(len(queries), tail_capacity=4)       # (outgrown by every query: the tails are re-allocated on the way)
    worst = 0.0
    with torch.inference_mode():
        pos = torch.zeros(len(queries), 1, dtype=torch.long, device=DEV)
        for b, q in enumerate(queries):
            fork.select_branch(b)
            p = torch.arange(base_len, base_len + q.shape[1], device=DEV).unsqueeze(0)
            lg = m.model(q.to(DEV), past_key_values=fork, use_cache=True, position_ids=p).logits[0, -1].float().cpu()
            want = seq[b][1][0]
            worst = max(worst, float((lg - want).abs().max() / want.abs().max()))
            assert (lg - want).abs().max() <= 1e-2 * want.abs().max(), (family, "first step", b)
            pos[b] = base_len + q.shape[1]
        for t in range(1, steps):
            cur = torch.cat([seq[b][0][t - 1] for b in range(len(queries))], dim=0)      # teacher forcing: the sequential tokens
            lg = m.model(cur, past_key_values=fork, use_cache=True, position_ids=pos).logits[:, -1].float().cpu()
            pos += 1
            for b in range(len(queries)):
                want = seq[b][1][t]
                worst = max(worst, float((lg[b] - want).abs().max() / want.abs().max()))
                assert (lg[b] - want).abs().max() <= 1e-2 * want.abs().max(), (family, "step", t, "branch", b)
    print(f"\nFORK model {family}: worst |logit difference| / max|logits| over {steps} steps x {len(queries)} branches: {worst:.2e}")
    assert fork.tail_len[0] == [q.shape[1] + steps - 1 for q in queries]


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_generate_batch(family):
    m, kv, queries = make(family)
    seen, off = kv.get_seq_length(), list(kv.info["offset"])
    k0 = kv.key_cache[0].clone()
    single = [m.generate(q, kv=kv, return_ids=True) for q in queries]
    batch = m.generate_batch(queries, kv, return_ids=True)
    assert len(batch) == len(queries)
    for a, b in zip(single, batch):
        assert b.shape == a.shape == (1, 5)        # max_new_tokens = 6, the last token dropped, as generate does
    # the base cache is as it was
    assert kv.get_seq_length() == seen and kv.info["offset"] == off
    again = [m.generate(q, kv=kv, return_ids=True) for q in queries]
    assert all(torch.equal(a, b) for a, b in zip(single, again))
    lens, seg = kv.info["len_k_host"][0], kv.info["seg_start"][0].tolist()
    for h in range(len(lens)):
        assert torch.equal(kv.key_cache[0][seg[h]:seg[h] + lens[h]], k0[seg[h]:seg[h] + lens[h]])
    # decoded text (no tokenizer: the ids as text), one string per query
    texts = m.generate_batch(queries, kv)
    assert len(texts) == 3 and all(isinstance(t, str) for t in texts)
    # more queries than one wave takes (G = 2: 16 branches per wave)
    many = m.generate_batch(queries * 6, kv, return_ids=True)
    assert len(many) == 18 and all(x.shape == (1, 5) for x in many)


def test_a_branch_that_meets_eos_stops_while_the_others_go_on():
    m, kv, queries = make("llama", max_new_tokens=8)
    ref = m.generate_batch(queries, kv, return_ids=True)
    assert all(x.shape[1] == 7 for x in ref)
    # EOS := a token the first branch is known to emit, picked so that (if any such token exists) another branch emits it later or
    # never: the first branch stops there, every other branch at its own first occurrence of the token or at the budget
    ids = [r[0].tolist() for r in ref]
    stop = lambda x, e: x.index(e) if e in x else len(x)  # noqa: E731  (the EOS itself is the dropped last token)
    cands = sorted(set(ids[0]), key=lambda e: -max(stop(x, e) - stop(ids[0], e) for x in ids[1:]))
    eos = cands[0]
    m.gen_kwargs["eos_token_id"] = eos
    out = m.generate_batch(queries, kv, return_ids=True)
    want = [x[:stop(x, eos)] for x in ids]
    print(f"\nFORK eos {eos}: answer lengths {[len(w) for w in want]} of {[len(x) for x in ids]}")
    assert [o[0].tolist() for o in out] == want
    assert len(want[0]) < len(ids[0])
    assert kv.get_seq_length() == 305 and kv.info["offset"] == [0, 0]
