"""CPU: the batched token loop of ``generate_batch / generate_samples / generate_multi`` on a scripted model (host logic only: no
attention runs and no library call is made).  The "model" is a deterministic function of the ids fed to each slot so far; the caches
are stand-ins that only keep books: a fake fork and a fake cache batch record the ``select_packed / select_branch / retire / commit``
calls.  What the three paths must give is what scripted ``generate`` gives for the same query, one query at a time."""
import types

import pytest
import torch

from kvzip_amd.kvcache import EvictCache
from kvzip_amd.wrapper import ModelKVzip

V = 50
CFG = types.SimpleNamespace(num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2)   # G = 4: 16 branches per launch
QUERIES = [[5, 1, 4], [2, 9], [7, 3, 8, 6, 1]]
CTX = [16, 21, 19]                # context lengths of the caches of generate_multi (the forked paths use the first)


def script(fed):
    """Last-position logits after the ids ``fed``: the argmax is a function of the last two ids and the parity of the count, and
    three more entries are non-zero so that a draw can land elsewhere."""
    x = torch.zeros(V)
    top = (3 * fed[-1] + 2 * fed[-2] + len(fed)) % 11
    for j in range(4):
        x[(top + 7 * j) % V] = 1.0 - 0.25 * j
    return x


class Books(EvictCache):
    """A pruned slack-layout EvictCache that holds no rows: ``fed`` lists the ids whose rows it would hold."""

    def get_seq_length(self, layer_idx=0):
        return self._seen_tokens

    def slice(self, seen):
        del self.fed[len(self.fed) - (self._seen_tokens - seen):]
        super().slice(seen)

    def feed(self, toks):
        self.fed += toks
        self._seen_tokens += len(toks)
        self.info["offset"] = [o + len(toks) for o in self.info["offset"]]


class FakeFork:
    layout = "fork"

    def __init__(self, base, n_branches):
        self.base, self.n_branches = base, n_branches
        self.shared = list(base.fed)                # the rows all branches see
        self.tails = [[] for _ in range(n_branches)]
        self.active = [True] * n_branches
        self._packed, self._branch = None, None
        self.steps = 0                              # batched decode forwards so far
        self.retired = []                           # (branch, steps when it was retired)
        self.committed = []

    def select_packed(self, branches, lengths):
        assert all(self.active[b] for b in branches) and len(set(branches)) == len(branches) == len(lengths)
        self._packed = (list(branches), list(lengths))

    def select_branch(self, b):
        self._branch = b

    def retire(self, b):
        self.retired.append((b, self.steps))
        self.active[b] = False

    def commit(self, b):
        self.committed.append(b)
        self.base.feed(self.tails[b])

    def history(self, b):
        return self.shared + self.tails[b]

    def feed(self, b, toks):
        self.tails[b] += toks


class FakeBatch:
    layout = "multi"
    made = []                                       # every batch built since the last _scripted()

    def __init__(self, caches):
        self.caches, self.n_caches = list(caches), len(caches)
        self.active = [True] * self.n_caches
        self._packed = None
        self.steps = 0
        self.retired = []
        FakeBatch.made.append(self)

    select_packed = FakeFork.select_packed
    retire = FakeFork.retire

    def history(self, b):
        return self.caches[b].fed

    def feed(self, b, toks):
        self.caches[b].feed(toks)


def _scripted(max_new_tokens=12, eos=None, sample_seed=None):
    """-> (ModelKVzip on the scripted model, its caches, the forks made, the forward passes run as (kind, batch, positions, position_ids))."""
    kvs, forks, calls = [], [], []
    FakeBatch.made = []
    for i, n in enumerate(CTX):
        kv = Books(CFG, (0, n), device="cpu", dtype=torch.float16, verbose=False)
        kv.pruned = True
        kv.info = {"flatten": True, "layout": "slack", "offset": [0, 0]}
        kv._seen_tokens = n
        kv.fed = [(7 * i + j) % 13 for j in range(n)]
        kv.prefill_ids = torch.tensor(kv.fed)[None]

        def fork(n_branches, tail_capacity=256, kv=kv):
            forks.append(FakeFork(kv, n_branches))
            return forks[-1]
        kv.fork = fork
        kvs.append(kv)

    def model(ids, past_key_values=None, use_cache=True, position_ids=None):
        c = past_key_values
        bsz, t = ids.shape
        logits = torch.zeros(bsz, t, V)
        if isinstance(c, Books):                                        # the sequential path: one query on one cache
            assert bsz == 1
            kind = "first"
            for i, tok in enumerate(ids[0].tolist()):
                c.feed([tok])
                logits[0, i] = script(c.fed)
        elif c._packed is not None:                                     # the first steps of several slots back to back
            assert bsz == 1
            kind = "packed"
            (slots, lengths), c._packed = c._packed, None
            assert t == sum(lengths)
            i = 0
            for b, n in zip(slots, lengths):
                for tok in ids[0, i:i + n].tolist():
                    c.feed(b, [tok])
                    logits[0, i] = script(c.history(b))
                    i += 1
        elif t == 1 and bsz == len(c.active):                           # one token for every live slot
            kind = "step"
            c.steps += 1
            for b in range(bsz):
                if c.active[b]:
                    c.feed(b, [int(ids[b, 0])])
                    logits[b, 0] = script(c.history(b))
        else:                                                           # the first step of the selected branch of a fork
            assert bsz == 1 and isinstance(c, FakeFork)
            kind = "first"
            for i, tok in enumerate(ids[0].tolist()):
                c.feed(c._branch, [tok])
                logits[0, i] = script(c.history(c._branch))
        calls.append((kind, bsz, t, None if position_ids is None else position_ids.tolist()))
        return types.SimpleNamespace(logits=logits)

    m = ModelKVzip.__new__(ModelKVzip)
    m.device, m.config, m.model, m.tokenizer = torch.device("cpu"), CFG, model, None
    m.gen_kwargs = {"do_sample": sample_seed is not None, "temperature": 1.0, "top_k": None, "top_p": 1, "max_new_tokens": max_new_tokens}
    if eos is not None:
        m.gen_kwargs["eos_token_id"] = eos
    m.sample_generator = None if sample_seed is None else torch.Generator().manual_seed(sample_seed)
    m.fork_max_branches, m.multi_max_caches, m.fork_packed_first, m.multi_packed_first = 16, 16, True, True
    return m, kvs, forks, calls


def _q(i):
    return torch.tensor([QUERIES[i]])


def _call(name, m, *a, **k):
    return getattr(ModelKVzip, name).__wrapped__.__wrapped__(m, *a, **k)


def _books(kv):
    return (kv._seen_tokens, list(kv.info["offset"]), list(kv.fed), kv.prefill_ids[0].tolist())


def _generate(q, cache, max_new, eos, update_cache=False):
    """What scripted ``generate`` answers to query ``q`` over cache ``cache``, and the cache's books afterwards."""
    m, kvs, _, _ = _scripted(max_new, eos)
    a = _call("generate", m, _q(q), kv=kvs[cache], update_cache=update_cache, return_ids=True)
    return a[0].tolist(), _books(kvs[cache])


@pytest.fixture(autouse=True)
def _fake_batch(monkeypatch):
    monkeypatch.setattr("kvzip_amd.wrapper.CacheBatch", FakeBatch)


# ---- the three paths, run once and described the same way ------------------------------------------------------------------------------
def _run(path, max_new, eos=None, packed=True, sample_seed=None, **kw):
    """-> (answers as lists, queries and caches (q, cache) per slot, first position per slot, the slot cache, calls, caches, books before)."""
    m, kvs, forks, calls = _scripted(max_new, eos, sample_seed)
    m.fork_packed_first = m.multi_packed_first = packed
    before = [_books(kv) for kv in kvs]
    if path == "batch":
        slots = [(i, 0) for i in range(3)]
        ans = _call("generate_batch", m, [_q(i) for i in range(3)], kvs[0], return_ids=True, **kw)
    elif path == "samples":
        slots = [(1, 0)] * 3
        ans = _call("generate_samples", m, _q(1), kvs[0], 3, return_ids=True)
    else:
        slots = [(i, i) for i in range(3)]
        ans = _call("generate_multi", m, [_q(i) for i in range(3)], kvs, return_ids=True, **kw)
    first_pos = [CTX[c] + len(QUERIES[q]) for q, c in slots]
    cache = forks[0] if path != "multi" else FakeBatch.made[0]
    assert len(forks) + len(FakeBatch.made) == 1
    assert all(a.dtype == torch.long and a.shape[0] == 1 for a in ans)
    return [a[0].tolist() for a in ans], slots, first_pos, cache, calls, kvs, before


PATHS = [("batch", True), ("batch", False), ("samples", True), ("multi", True), ("multi", False)]
IDS = [f"{p}-{'packed' if k else 'per-slot'}" for p, k in PATHS]


def _check_against_generate(path, packed, max_new, eos):
    ans, slots, first_pos, cache, calls, kvs, before = _run(path, max_new, eos, packed)
    want = [_generate(q, c, max_new, eos)[0] for q, c in slots]
    assert ans == want, (path, packed, max_new, eos)
    n_tok = [len(w) + 1 for w in want]                                   # tokens a slot produced, the dropped last one included
    # a slot is retired exactly once, after the step that gave its last token, while the others go on
    assert sorted(cache.retired) == [(b, n - 1) for b, n in enumerate(n_tok)], (path, packed, max_new, eos)
    steps = [c for c in calls if c[0] == "step"]
    assert len(steps) == max(n_tok) - 1 == cache.steps
    for s, (_, bsz, t, pos) in enumerate(steps):
        assert (bsz, t) == (3, 1) and pos == [[p + s] for p in first_pos]
    assert [_books(kv) for kv in kvs] == before                          # nothing is kept: every cache's books are where they were
    return calls


@pytest.mark.parametrize("path,packed", PATHS, ids=IDS)
def test_greedy_answers_are_generates_at_every_budget(path, packed):
    for max_new in (1, 2, 7, 12):
        _check_against_generate(path, packed, max_new, None)


@pytest.mark.parametrize("path,packed", PATHS, ids=IDS)
def test_a_slot_stops_at_eos_while_the_others_go_on(path, packed):
    full = [_generate(q, c, 12, None)[0] for q, c in ((0, 0), (1, 0), (2, 0), (1, 1), (2, 2))]
    seen = sorted({t for a in full for t in a})
    assert len(seen) >= 4
    for eos in seen:
        _check_against_generate(path, packed, 12, eos)
    _check_against_generate(path, packed, 12, seen[:3])                  # (a list of EOS ids)
    for max_new in (1, 2, 7):
        _check_against_generate(path, packed, max_new, seen[1])


def test_the_eos_cases_end_slots_at_different_steps():
    """(the check above is only worth something if the slots do not all stop together)"""
    ragged = 0
    full = sorted({t for q in range(3) for t in _generate(q, 0, 12, None)[0]})
    for eos in full:
        n = [len(_generate(q, 0, 12, eos)[0]) for q in range(3)]
        ragged += len(set(n)) > 1
    assert ragged >= 2


# ---- the first step ---------------------------------------------------------------------------------------------------------------------
def test_packed_first_step_of_a_fork_sits_behind_the_context():
    _, _, _, cache, calls, _, _ = _run("batch", 4, packed=True)
    lens = [len(q) for q in QUERIES]
    assert calls[0] == ("packed", 1, sum(lens), [[CTX[0] + i for n in lens for i in range(n)]])
    assert [c[0] for c in calls[1:]] == ["step"] * (len(calls) - 1)
    assert cache.tails[1][:2] == QUERIES[1]


def test_packed_first_step_of_a_batch_sits_behind_every_cache_of_its_own():
    _, _, _, _, calls, _, _ = _run("multi", 4, packed=True)
    lens = [len(q) for q in QUERIES]
    assert calls[0] == ("packed", 1, sum(lens), [[CTX[b] + i for b, n in enumerate(lens) for i in range(n)]])
    assert [c[0] for c in calls[1:]] == ["step"] * (len(calls) - 1)


def test_per_slot_first_steps():
    _, _, _, _, calls, _, _ = _run("batch", 4, packed=False)
    assert calls[:3] == [("first", 1, len(q), [list(range(CTX[0], CTX[0] + len(q)))]) for q in QUERIES]
    _, _, _, _, calls, _, _ = _run("multi", 4, packed=False)
    assert calls[:3] == [("first", 1, len(q), None) for q in QUERIES]    # (a cache's own path knows its positions)
    _, _, _, _, calls, _, _ = _run("samples", 4)
    assert calls[0] == ("first", 1, len(QUERIES[1]), None) and [c[0] for c in calls[1:]] == ["step"] * 3


def test_more_slots_than_a_wave_takes():
    for packed in (True, False):
        m, kvs, forks, calls = _scripted(7)
        m.fork_max_branches, m.fork_packed_first = 2, packed
        ans = _call("generate_batch", m, [_q(i) for i in range(3)], kvs[0], return_ids=True)
        assert [a[0].tolist() for a in ans] == [_generate(q, 0, 7, None)[0] for q in range(3)]
        assert [f.n_branches for f in forks] == [2, 1]
        ans = _call("generate_samples", m, _q(2), kvs[0], 5, return_ids=True)
        assert [a[0].tolist() for a in ans] == [_generate(2, 0, 7, None)[0]] * 5
        assert [f.n_branches for f in forks[2:]] == [2, 2, 1] and sum(c[0] == "first" and c[3] is None for c in calls) == 1


# ---- the order of the draws --------------------------------------------------------------------------------------------------------------
def _replay(histories, gen_kwargs, seed):
    """The batched loop as the draws see it: first token of slots 0 .. B-1, then per step the live slots in slot order."""
    g = torch.Generator().manual_seed(seed)
    eos = gen_kwargs.get("eos_token_id", [])
    hist, out, live = [list(h) for h in histories], [[] for _ in histories], [True] * len(histories)

    def take(b):
        tok = int(ModelKVzip.next_token(script(hist[b])[None], gen_kwargs, g))
        out[b].append(tok)
        live[b] = tok not in eos and len(out[b]) < gen_kwargs["max_new_tokens"]

    for b in range(len(hist)):
        take(b)
    while any(live):
        for b in range(len(hist)):
            if live[b]:
                hist[b].append(out[b][-1])
                take(b)
    return [o[:-1] for o in out]


@pytest.mark.parametrize("path,packed", PATHS, ids=IDS)
def test_draws_come_in_slot_order(path, packed):
    ragged = 0
    for seed in range(6):
        ans, slots, _, _, _, kvs, before = _run(path, 9, eos=[0, 7, 14, 21], packed=packed, sample_seed=seed)
        m, kvs0, _, _ = _scripted(9, [0, 7, 14, 21], sample_seed=seed)
        assert ans == _replay([kvs0[c].fed + QUERIES[q] for q, c in slots], m.gen_kwargs, seed), (path, packed, seed)
        assert [_books(kv) for kv in kvs] == before
        ragged += len({len(a) for a in ans}) > 1
        greedy = [_generate(q, c, 9, [0, 7, 14, 21])[0] for q, c in slots]
        ragged += 10 * (ans != greedy)
    assert ragged % 10 >= 1 and ragged >= 10       # slots ended at different steps, and a draw left the greedy path


# ---- how a turn ends ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "per-slot"])
def test_keep_leaves_the_cache_as_generate_with_update_cache(packed):
    for max_new, eos in ((1, None), (7, None), (12, 3)):
        for keep in range(3):
            ans, _, _, cache, _, kvs, before = _run("batch", max_new, eos, packed, keep=keep)
            want, books = _generate(keep, 0, max_new, eos, update_cache=True)
            assert ans[keep] == want and cache.committed == [keep]
            assert _books(kvs[0]) == books and books[2] == before[0][2] + QUERIES[keep] + want == books[3]


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "per-slot"])
def test_generate_multi_update_cache_leaves_every_cache_as_generate_does(packed):
    for max_new, eos in ((1, None), (7, None), (12, 3)):
        ans, slots, _, _, _, kvs, before = _run("multi", max_new, eos, packed, update_cache=True)
        for b, (q, c) in enumerate(slots):
            want, books = _generate(q, c, max_new, eos, update_cache=True)
            assert ans[b] == want and _books(kvs[c]) == books and books[3] == before[c][3] + QUERIES[q] + want
