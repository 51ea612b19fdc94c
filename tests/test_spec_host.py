"""CPU: the host side of speculative decoding - the prompt-lookup drafter and the greedy acceptance rule (kvzip_amd/draft.py)."""
import torch

from kvzip_amd.draft import accept_greedy, lookup_draft


def ids(*x):
    return torch.tensor(x, dtype=torch.long)


def test_latest_match_wins_over_an_earlier_one():
    #            0  1  2  3  4  5  6  7  8  9
    h = ids(1, 2, 3, 50, 51, 1, 2, 3, 60, 61, 62, 9, 1, 2, 3)
    assert lookup_draft(h, 2).tolist() == [60, 61]
    assert lookup_draft(h, 3).tolist() == [60, 61, 62]
    assert lookup_draft(h, 1, ngram_max=1).tolist() == [60]          # the latest earlier 3 is the one before 60


def test_longer_ngram_wins_over_the_shorter():
    # the last id alone (7) occurs latest before 90; the last two ids (6, 7) occur before 80: the 2-gram decides
    h = ids(6, 7, 80, 81, 5, 7, 90, 91, 6, 7)
    assert lookup_draft(h, 2, ngram_max=3).tolist() == [80, 81]      # no 3-gram match (5, 6, 7 never occurred): falls to 2
    assert lookup_draft(h, 2, ngram_max=1).tolist() == [90, 91]
    assert lookup_draft(h, 2, ngram_max=3, ngram_min=3).numel() == 0


def test_continuation_that_runs_into_the_end_is_shorter():
    h = ids(4, 5, 6, 4, 5)
    assert lookup_draft(h, 8).tolist() == [6, 4, 5]                  # everything behind the match, which is fewer than 8 ids
    h = ids(3, 3)
    assert lookup_draft(h, 4).tolist() == [3]                        # the only earlier occurrence is followed by the last id alone


def test_no_match_gives_an_empty_draft():
    h = ids(1, 2, 3, 4, 5)
    d = lookup_draft(h, 4)
    assert d.numel() == 0 and d.dtype == torch.long and d.dim() == 1
    assert lookup_draft(ids(1, 2, 1), 0).numel() == 0                # nothing asked for
    # the end of the history is no occurrence of itself
    assert lookup_draft(ids(1, 2, 3), 4, ngram_max=3, ngram_min=3).numel() == 0


def test_history_shorter_than_the_ngram():
    assert lookup_draft(ids(), 4).numel() == 0
    assert lookup_draft(ids(7), 4).numel() == 0
    assert lookup_draft(ids(7, 7), 4, ngram_max=3).tolist() == [7]   # only the 1-gram fits
    assert lookup_draft(ids(7, 8, 7, 8), 4, ngram_max=5).tolist() == [7, 8]   # 5-, 4- and 3-grams do not fit; the 2-gram matches


def test_long_history_without_a_python_loop_over_the_ids():
    g = torch.Generator().manual_seed(0)
    h = torch.randint(0, 50000, (131072,), generator=g)
    h[1000:1004] = torch.tensor([11, 12, 13, 14])
    h[-3:] = torch.tensor([11, 12, 13])
    h[70000:70003] = torch.tensor([11, 12, 99])                      # a later 2-gram match that is no 3-gram match
    assert lookup_draft(h, 1).tolist() == [14]
    assert lookup_draft(h.view(1, -1), 1).tolist() == [14]           # (a [1, n] tensor is taken as its row)


def test_accept_greedy():
    am = ids(5, 6, 7, 8)                                              # the model's argmax at the 4 positions of [last, d0, d1, d2]
    assert accept_greedy(ids(5, 6, 7), am) == 3                      # all
    assert accept_greedy(ids(9, 6, 7), am) == 0                      # none: later agreements do not count
    assert accept_greedy(ids(5, 6, 9), am) == 2                      # a prefix
    assert accept_greedy(ids(5, 9, 7), am) == 1
    assert accept_greedy(ids(), am) == 0                             # an empty draft
    assert accept_greedy(ids(5), ids(5)) == 1
    assert isinstance(accept_greedy(ids(5, 6), am), int)


# ---- the speculative loop on a scripted model (host logic only: no attention runs) ------------------------------------------------------
V = 50


def _scripted(max_new_tokens=12, eos=None):
    """A ModelKVzip whose "model" is a deterministic function of all ids fed so far, over an EvictCache that only keeps the books."""
    import types
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
    kv.info = {"flatten": True, "layout": "slack", "offset": [0, 0]}
    kv._seen_tokens = 16
    kv.fed = list(range(16))
    kv.prefill_ids = torch.arange(16)[None]
    calls = []

    def model(ids, past_key_values=None, use_cache=True, position_ids=None):
        kv = past_key_values
        t = ids.shape[1]
        calls.append((t, bool(getattr(kv, "_verifying", False))))
        if position_ids is not None:
            assert position_ids[0].tolist() == list(range(kv._seen_tokens, kv._seen_tokens + t))
        logits = torch.zeros(1, t, V)
        for i, tok in enumerate(ids[0].tolist()):
            kv.fed.append(tok)
            # (a short period so that prompt lookup finds something to quote)
            logits[0, i, (3 * kv.fed[-1] + kv.fed[-2] + len(kv.fed) % 2) % 7] = 1.0
        kv._seen_tokens += t
        kv.info["offset"] = [o + t for o in kv.info["offset"]]
        return types.SimpleNamespace(logits=logits)

    m = ModelKVzip.__new__(ModelKVzip)
    m.device, m.config, m.model, m.tokenizer = torch.device("cpu"), cfg, model, None
    m.gen_kwargs = {"do_sample": False, "max_new_tokens": max_new_tokens}
    if eos is not None:
        m.gen_kwargs["eos_token_id"] = eos
    m.sample_generator = None
    return m, kv, calls


def _gen(m, *a, **k):
    from kvzip_amd.wrapper import ModelKVzip
    return ModelKVzip.generate.__wrapped__.__wrapped__(m, *a, **k)


def _spec(m, *a, **k):
    from kvzip_amd.wrapper import ModelKVzip
    return ModelKVzip.generate_speculative.__wrapped__.__wrapped__(m, *a, **k)


def test_speculative_loop_on_a_scripted_model():
    """Same ids as generate for every drafter, budget and EOS position; the cache's books end where generate leaves them."""
    q = torch.tensor([[5, 1, 4]])
    for max_new in (1, 2, 3, 7, 12):
        m, kv, _ = _scripted(max_new)
        ref = _gen(m, q, kv=kv, return_ids=True)
        assert ref.shape == (1, max_new - 1) and kv._seen_tokens == 16 and kv.info["offset"] == [0, 0] and kv.fed == list(range(16))
        full = ref[0].tolist()
        drafters = {
            "lookup": None,
            "right": lambda h, n: torch.tensor(full[h.shape[0] - 19:h.shape[0] - 19 + n], dtype=torch.long),
            "wrong": lambda h, n: torch.full((n,), V - 1, dtype=torch.long),
            "one right": lambda h, n: torch.tensor((full[h.shape[0] - 19:h.shape[0] - 18] + [V - 1] * n)[:n], dtype=torch.long),
            "too many": lambda h, n: torch.tensor(full[h.shape[0] - 19:] + [V - 1] * 9, dtype=torch.long),
            "empty": lambda h, n: torch.zeros(0, dtype=torch.long),
        }
        for name, d in drafters.items():
            for nd in (None, 1, 4, 100):
                m, kv, calls = _scripted(max_new)
                ids, st = _spec(m, q, kv, draft=d, num_draft=nd, return_ids=True, return_stats=True)
                assert ids[0].tolist() == full, (max_new, name, nd)
                assert kv._seen_tokens == 16 and kv.info["offset"] == [0, 0] and kv.fed == list(range(16)), (max_new, name, nd)
                assert st["tokens"] == max_new - 1 and st["accepted"] <= st["drafted"] and st["steps"] <= st["tokens"]
                assert all(v == (t > 1) for t, v in calls[1:]) and calls[0] == (3, False)
                assert all(t <= 1 + m._draft_len(nd) for t, _ in calls[1:])
                if name == "wrong":
                    assert st["accepted"] == 0 and st["steps"] == st["tokens"]
                if name == "empty":
                    assert st["drafted"] == 0 and all(t == 1 for t, _ in calls[1:])
                if name == "right" and max_new > 2:
                    assert st["accepted"] == st["drafted"] > 0 and st["steps"] < st["tokens"]
                # update_cache=True: the query and the answer stay, as after generate
                m, kv, _ = _scripted(max_new)
                _spec(m, q, kv, draft=d, num_draft=nd, update_cache=True)
                m2, kv2, _ = _scripted(max_new)
                _gen(m2, q, kv=kv2, update_cache=True)
                assert kv.fed == kv2.fed == list(range(16)) + [5, 1, 4] + full and kv._seen_tokens == kv2._seen_tokens
                assert kv.info["offset"] == kv2.info["offset"] and torch.equal(kv.prefill_ids, kv2.prefill_ids)


def test_speculative_loop_stops_at_eos_like_generate():
    q = torch.tensor([[5, 1, 4]])
    m, kv, _ = _scripted(12)
    full = _gen(m, q, kv=kv, return_ids=True)[0].tolist()
    for eos in sorted(set(full)):
        m, kv, _ = _scripted(12, eos=eos)
        want = _gen(m, q, kv=kv, return_ids=True)[0].tolist()
        assert want == full[:full.index(eos)]
        for d in (None, lambda h, n: torch.tensor(full[h.shape[0] - 19:h.shape[0] - 19 + n], dtype=torch.long)):
            for nd in (1, 3, 100):
                m, kv, _ = _scripted(12, eos=eos)
                assert _spec(m, q, kv, draft=d, num_draft=nd, return_ids=True)[0].tolist() == want
                assert kv.fed == list(range(16)) and kv.info["offset"] == [0, 0]
                _spec(m, q, kv, draft=d, num_draft=nd, update_cache=True)
                assert kv.fed == list(range(16)) + [5, 1, 4] + want and kv.info["offset"] == [3 + len(want)] * 2
