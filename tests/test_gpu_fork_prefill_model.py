"""GPU: the packed first step through the model (tiny random-init Llama / Qwen2 of tests/test_gpu_fork_model.py's sizes): ONE forward
pass over the queries of all branches against the sequential generate, and ModelKVzip.generate_batch with and without it."""
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
    """One packed first pass over the three queries (11 + 3, 4 + 3 and 23 + 3 tokens after the template), then four batched decode
    steps fed the token ids the sequential path produced: every branch's logits within 1e-2 x max|logits| of the sequential path's
    (the bound tests/test_gpu_fork_model.py takes for the per-branch first steps)."""
    m, kv, queries = make(family)
    assert [q.shape[1] for q in queries] == [14, 7, 26]
    steps = 5
    seq = [_sequential_logits(m, kv, q, steps) for q in queries]
    base_len = kv.get_seq_length()
    B = len(queries)
    fork = kv.fork(B, tail_capacity=4)       # (outgrown by the packed pass: the tails are re-allocated on the way)
    lens = [q.shape[1] for q in queries]
    worst = 0.0
    with torch.inference_mode():
        fork.select_packed(list(range(B)), lens)
        p = torch.cat([torch.arange(base_len, base_len + n, device=DEV) for n in lens]).unsqueeze(0)
        logits = m.model(torch.cat([q.to(DEV) for q in queries], dim=1), past_key_values=fork, use_cache=True, position_ids=p).logits
        assert fork._packed is None and logits.shape[:2] == (1, sum(lens))
        pos = torch.zeros(B, 1, dtype=torch.long, device=DEV)
        end = 0
        for b, n in enumerate(lens):
            end += n
            lg, want = logits[0, end - 1].float().cpu(), seq[b][1][0]
            worst = max(worst, float((lg - want).abs().max() / want.abs().max()))
            assert (lg - want).abs().max() <= 1e-2 * want.abs().max(), (family, "packed first step", b)
            pos[b] = base_len + n
        for t in range(1, steps):
            cur = torch.cat([seq[b][0][t - 1] for b in range(B)], dim=0)      # teacher forcing: the sequential tokens
            lg = m.model(cur, past_key_values=fork, use_cache=True, position_ids=pos).logits[:, -1].float().cpu()
            pos += 1
            for b in range(B):
                want = seq[b][1][t]
                worst = max(worst, float((lg[b] - want).abs().max() / want.abs().max()))
                assert (lg[b] - want).abs().max() <= 1e-2 * want.abs().max(), (family, "step", t, "branch", b)
    print(f"\nPREFILL model {family}: worst |logit difference| / max|logits| over {steps} steps x {B} branches: {worst:.2e}")
    assert fork.tail_len[0] == [q.shape[1] + steps - 1 for q in queries]


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_generate_batch_packs_the_first_steps(family, monkeypatch):
    """fork_packed_first True and False: both leave the base cache untouched and return answers of the same shapes; the packed run
    makes exactly ONE first-step forward per wave (ForkedCache.first_step calls per layer, counted by a wrapper)."""
    from kvzip_amd.kvcache import ForkedCache
    m, kv, queries = make(family)
    assert m.fork_packed_first is True
    seen, off = kv.get_seq_length(), list(kv.info["offset"])
    k0, v0 = kv.key_cache[0].clone(), kv.value_cache[0].clone()
    calls = []
    real = ForkedCache.first_step

    def counted(self, query_states, key_states, value_states, layer_idx, softmax_scale=None):
        calls.append((layer_idx, query_states.shape[2]))
        return real(self, query_states, key_states, value_states, layer_idx, softmax_scale=softmax_scale)
    monkeypatch.setattr(ForkedCache, "first_step", counted)

    def per_layer():
        n = [sum(1 for l, _ in calls if l == layer) for layer in range(kv.n_layers)]
        assert len(set(n)) == 1
        return n[0]
    lens = [q.shape[1] for q in queries]
    packed = m.generate_batch(queries, kv, return_ids=True)
    assert per_layer() == 1 and {t for _, t in calls} == {sum(lens)}              # one wave: one packed forward
    del calls[:]
    many = m.generate_batch(queries * 6, kv, return_ids=True)                      # G = 2: 16 branches per wave -> two waves
    assert per_layer() == 2 and len(many) == 18
    del calls[:]
    one = m.generate_batch(queries[:1], kv, return_ids=True)                       # a wave of one query: the per-branch path
    assert per_layer() == 1 and calls[0][1] == lens[0] and one[0].shape == (1, 5)
    del calls[:]
    m.fork_packed_first = False
    loop = m.generate_batch(queries, kv, return_ids=True)
    assert per_layer() == 3 and [t for l, t in calls if l == 0] == lens            # one forward per branch, as before
    assert len(packed) == len(loop) == 3
    for a, b in zip(packed, loop):
        assert a.shape == b.shape == (1, 5)        # max_new_tokens = 6, the last token dropped, as generate does
    assert all(x.shape == (1, 5) for x in many)
    # the base cache is as it was
    assert kv.get_seq_length() == seen and kv.info["offset"] == off
    lens_k, seg = kv.info["len_k_host"][0], kv.info["seg_start"][0].tolist()
    for h in range(len(lens_k)):
        sl = slice(seg[h], seg[h] + lens_k[h])
        assert torch.equal(kv.key_cache[0][sl], k0[sl]) and torch.equal(kv.value_cache[0][sl], v0[sl])
