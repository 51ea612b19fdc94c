"""GPU: the packed first step of generate_multi through the model (tiny random-init Llama / Qwen2 of tests/test_gpu_multi_model.py):
ONE forward pass over the queries of all caches against the sequential first step on clones, and ModelKVzip.generate_multi with
``multi_packed_first`` on against off."""
import pytest
import torch

from test_gpu_multi_model import _sequential_logits, make

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-2        # x max|logits|: the bound of tests/test_gpu_multi_model.py


def _packed_teacher_forced(m, kvs, clones, queries, steps):
    """Worst |logit difference| / max|logits| of ONE packed first pass and `steps - 1` batched decode steps fed the tokens the
    sequential path produced on the clones; asserts the bound.  The caches are sliced back."""
    from kvzip_amd.kvcache import CacheBatch
    seq = [_sequential_logits(m, c, q, steps) for c, q in zip(clones, queries)]
    seen = [kv._seen_tokens for kv in kvs]
    B = len(kvs)
    lens = [q.shape[1] for q in queries]
    batch = CacheBatch(kvs)
    worst = 0.0
    with torch.inference_mode():
        batch.select_packed(list(range(B)), lens)
        p = torch.cat([torch.arange(s, s + n, device=DEV) for s, n in zip(seen, lens)]).unsqueeze(0)
        logits = m.model(torch.cat([q.to(DEV) for q in queries], dim=1), past_key_values=batch, use_cache=True, position_ids=p).logits
        assert batch._packed is None and logits.shape[:2] == (1, sum(lens))
        pos = torch.zeros(B, 1, dtype=torch.long, device=DEV)
        end = 0
        for b, n in enumerate(lens):
            end += n
            lg, want = logits[0, end - 1].float().cpu(), seq[b][1][0]
            worst = max(worst, float((lg - want).abs().max() / want.abs().max()))
            assert (lg - want).abs().max() <= BOUND * want.abs().max(), ("packed first step", b)
            assert kvs[b].get_seq_length() == seen[b] + n and kvs[b].info["offset"] == [n] * 2
            pos[b] = kvs[b].get_seq_length()
        for t in range(1, steps):
            cur = torch.cat([seq[b][0][t - 1] for b in range(B)], dim=0)      # teacher forcing: the sequential tokens
            lg = m.model(cur, past_key_values=batch, use_cache=True, position_ids=pos).logits[:, -1].float().cpu()
            pos += 1
            for b in range(B):
                want = seq[b][1][t]
                worst = max(worst, float((lg[b] - want).abs().max() / want.abs().max()))
                assert (lg[b] - want).abs().max() <= BOUND * want.abs().max(), ("step", t, "cache", b)
    for kv, q, s in zip(kvs, queries, seen):
        assert kv.info["offset"] == [q.shape[1] + steps - 1] * 2 and kv._seen_tokens == s + q.shape[1] + steps - 1
        kv.slice(s)
    return worst


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_packed_first_step_logits_match_the_sequential_path(family):
    """The packed pass over the two queries (11 + 3 and 4 + 3 tokens after the template), every cache at its own positions, then three
    teacher-forced batched steps: every cache's logits within 1e-2 x max|logits| of the sequential path's on its clone."""
    m, kvs, clones, queries = make(family)
    assert [q.shape[1] for q in queries] == [14, 7]
    worst = _packed_teacher_forced(m, kvs, clones, queries, 4)
    print(f"\nMULTI-PREFILL model {family}: worst |logit difference| / max|logits| over 4 steps x 2 caches: {worst:.2e}")


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_generate_multi_packed_against_sequential_first_steps(family, monkeypatch):
    """multi_packed_first on against off: token ids of at least one of the two sequences identical (the packed first step sums in
    another order: where a sequence's ids differ, the teacher-forced logits must agree instead); the packed run makes exactly ONE
    first-step call per layer; the caches are ordinary EvictCache objects again afterwards."""
    from kvzip_amd.kvcache import CacheBatch
    m, kvs, clones, queries = make(family)
    assert m.multi_packed_first is True
    seen = [kv.get_seq_length() for kv in kvs]
    calls = []
    real = CacheBatch.first_step

    def counted(self, query_states, key_states, value_states, layer_idx, softmax_scale=None):
        calls.append((layer_idx, query_states.shape[2]))
        return real(self, query_states, key_states, value_states, layer_idx, softmax_scale=softmax_scale)
    monkeypatch.setattr(CacheBatch, "first_step", counted)
    packed = m.generate_multi(queries, kvs, return_ids=True)
    assert calls == [(0, 21), (1, 21)]                           # one packed forward: one call per layer, 14 + 7 positions
    del calls[:]
    m.multi_packed_first = False
    loop = m.generate_multi(queries, clones, return_ids=True)
    assert calls == []                                           # one forward per cache on its own path, as before
    m.multi_packed_first = True
    assert all(a.shape == b.shape == (1, 5) for a, b in zip(packed, loop))    # max_new_tokens = 6, the last dropped
    same = [torch.equal(a, b) for a, b in zip(packed, loop)]
    print(f"\nMULTI-PREFILL generate {family}: identical token ids per sequence: {same}")
    assert any(same)
    if not all(same):
        _packed_teacher_forced(m, kvs, clones, queries, 4)
    # every cache is as it was, and an ordinary EvictCache again
    for kv, c, s in zip(kvs, clones, seen):
        assert kv.get_seq_length() == s == c.get_seq_length() and kv.info["offset"] == [0, 0]
    single = [m.generate(q, kv=c, return_ids=True) for q, c in zip(queries, clones)]
    again = [m.generate(q, kv=kv, return_ids=True) for q, kv in zip(queries, kvs)]
    assert all(torch.equal(a, b) for a, b in zip(single, again))
    one = m.generate_multi(queries[:1], kvs[:1], return_ids=True)             # a wave of one: the sequential path
    assert calls == [] and torch.equal(one[0], single[0])


def test_update_cache_keeps_the_turn():
    """update_cache=True after a packed first step: both caches hold the query and the answer afterwards (offsets, lengths,
    prefill_ids) as the clones do after their own generate(update_cache=True)."""
    m, kvs, clones, queries = make("qwen2")
    single = [m.generate(q, kv=c, update_cache=True, return_ids=True) for q, c in zip(queries, clones)]
    multi = m.generate_multi(queries, kvs, update_cache=True, return_ids=True)
    same = [torch.equal(a, b) for a, b in zip(multi, single)]
    print(f"\nMULTI-PREFILL update_cache: turn identical {same}")
    for kv, c, a, q in zip(kvs, clones, multi, queries):
        assert kv.info["offset"] == c.info["offset"] == [q.shape[1] + 5] * 2 and kv.get_seq_length() == c.get_seq_length()
        assert kv.prefill_ids.shape == c.prefill_ids.shape and torch.equal(kv.prefill_ids[:, -5:], a)
        assert torch.equal(kv.prefill_ids[:, -5 - q.shape[1]:-5].cpu(), q.cpu())
