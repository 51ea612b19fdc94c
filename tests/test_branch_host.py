"""CPU: kvcache.plan_branch_reorder - where the hypotheses of a beam-search step live and which tails are copied for it - over every
parent vector of up to 4 slots and fixed cases at 16, and what ForkedCache.reorder / commit refuse (host logic only; the fork is put
together by hand)."""
import itertools
import types

import pytest

from kvzip_amd.kvcache import ForkedCache, plan_branch_reorder


def _check_plan(parents, n_slots):
    slots, pairs = plan_branch_reorder(parents, n_slots)
    assert (slots, pairs) == plan_branch_reorder(list(parents), n_slots)              # deterministic
    assert len(slots) == len(parents) and all(0 <= s < n_slots for s in slots)
    assert len(set(slots)) == len(slots)                                                # injective: one hypothesis per slot
    # play the copies on "what slot s holds": hypothesis i's content comes from parents[i]
    content = list(range(n_slots))
    before = list(content)
    for s, d in pairs:
        content[d] = before[s]
    assert [content[s] for s in slots] == list(parents)
    # a parent's slot keeps one of its children - the first - and no copy is made for it
    for p in set(parents):
        first = list(parents).index(p)
        assert slots[first] == p
    srcs, dsts = {s for s, _ in pairs}, [d for _, d in pairs]
    assert not srcs & set(dsts) and len(set(dsts)) == len(dsts)                        # disjoint sides, every destination once
    assert srcs <= set(parents) and not set(dsts) & set(parents)                       # destinations are childless slots
    # one copy per child beyond a parent's first = the childless slots that get reused, lowest slot first
    childless = [s for s in range(n_slots) if s not in set(parents)]
    assert len(pairs) == len(parents) - len(set(parents))
    assert dsts == childless[:len(pairs)]
    if len(parents) == n_slots:
        assert len(pairs) == len(childless)                                              # all slots in use: the dropped hypotheses
    return slots, pairs


def test_every_parent_vector_up_to_four_slots():
    n = 0
    for n_slots in range(1, 5):
        for k in range(0, n_slots + 1):
            for parents in itertools.product(range(n_slots), repeat=k):
                _check_plan(parents, n_slots)
                n += 1
    assert n == 2 + 7 + 40 + 341


def test_fixed_cases_at_sixteen_slots():
    ident = list(range(16))
    assert _check_plan(ident, 16) == (ident, [])
    rev = ident[::-1]
    assert _check_plan(rev, 16) == (rev, [])                                            # a permutation of survivors costs nothing
    slots, pairs = _check_plan([7] * 16, 16)                                            # one parent feeds everybody
    assert slots == [7] + [s for s in range(16) if s != 7] and pairs == [(7, d) for d in range(16) if d != 7]
    slots, pairs = _check_plan([3, 3, 9, 0, 9, 9, 15, 1, 2, 4, 5, 6, 8, 10, 11, 12], 16)
    assert pairs == [(3, 7), (9, 13), (9, 14)] and slots[:7] == [3, 7, 9, 0, 13, 14, 15]
    slots, pairs = _check_plan([15, 15, 0], 16)                                         # fewer hypotheses than slots
    assert slots == [15, 1, 0] and pairs == [(15, 1)]
    assert _check_plan([], 16) == ([], [])


def test_plan_refuses_bad_input():
    with pytest.raises(ValueError, match="5 hypotheses for 4 slots"):
        plan_branch_reorder([0, 1, 2, 3, 0], 4)
    with pytest.raises(ValueError, match="outside"):
        plan_branch_reorder([0, 4], 4)
    with pytest.raises(ValueError, match="outside"):
        plan_branch_reorder([-1], 4)


# ---- ForkedCache.reorder / commit: what they refuse and the bookkeeping they leave (no rows held: nothing is launched) --------------------
def _fork(n=4, n_layers=2, tail_len=0):
    f = ForkedCache.__new__(ForkedCache)
    f.base = types.SimpleNamespace(_layout_epoch=0, info={"flatten": True, "offset": [0] * n_layers}, slack=8, _seen_tokens=100)
    f.n_branches, f.n_layers, f.n_heads_kv, f.n_group_kv = n, n_layers, 2, 2
    f._epoch, f._offset = 0, [0] * n_layers
    f.tail_k, f.tail_v = [None] * n_layers, [None] * n_layers
    f.tail_len = [[tail_len] * n for _ in range(n_layers)]
    f.active = [True] * n
    f._packed = None
    return f


def test_reorder_bookkeeping_and_refusals():
    from kvzip_amd.ops import KvzError
    f = _fork()
    assert f.reorder([2, 2, 0]) == [2, 1, 0]                 # (empty tails: the plan is applied, nothing is copied)
    assert f.active == [True, True, True, False]             # slot 3 is left without a hypothesis: retired
    with pytest.raises(KvzError, match="branch 3 is retired"):
        f.reorder([3])
    with pytest.raises(KvzError, match="no branch 4"):
        f.reorder([4])
    with pytest.raises(KvzError, match="5 hypotheses"):
        f.reorder([0, 0, 0, 0, 0])
    assert f.reorder([1, 1, 1, 1]) == [1, 0, 2, 3] and f.active == [True] * 4
    f.select_packed([0, 1], [3, 4])
    with pytest.raises(KvzError, match="packing is selected"):
        f.reorder([0])
    with pytest.raises(KvzError, match="packing is selected"):
        f.commit(0)
    f._packed = None
    f.tail_len[1][2] = 5                                      # layer 1 is one forward pass ahead of layer 0
    with pytest.raises(KvzError, match="middle of a forward pass"):
        f.reorder([2, 2])
    assert f.reorder([2, 0]) == [2, 0]                        # (no copy planned: nothing to compare)
    f.base._layout_epoch = 1
    with pytest.raises(KvzError, match="re-laid out"):
        f.reorder([0])


def test_commit_closes_the_fork():
    from kvzip_amd.ops import KvzError
    f = _fork()
    with pytest.raises(KvzError, match="no branch 7"):
        f.commit(7)
    f.base.info["offset"] = [3, 3]
    with pytest.raises(KvzError, match="appended to the base cache since the fork"):
        f.commit(1)
    f.base.info["offset"] = [0, 0]
    f.commit(1)                                               # an empty tail: nothing to append, the fork closes all the same
    assert f.base.info["offset"] == [0, 0] and f.base._seen_tokens == 100
    for hook in (lambda: f.reorder([0]), lambda: f.commit(0), lambda: f.first_step(None, None, None, 0),
                 lambda: f.update_attend(None, None, None, 0)):
        with pytest.raises(KvzError, match="closed"):
            hook()


def test_wrapper_limits_and_keep_refusals():
    from kvzip_amd.ops import KvzError
    from kvzip_amd.wrapper import ModelKVzip
    m = ModelKVzip.__new__(ModelKVzip)
    m.config = types.SimpleNamespace(num_attention_heads=28, num_key_value_heads=4)     # G = 7: 9 branches per launch
    m._fork_limit("generate_beam", 9)
    with pytest.raises(KvzError, match="at most 64 query rows.*at most 16 branches"):
        m._fork_limit("generate_beam", 10)
    m.config = types.SimpleNamespace(num_attention_heads=4, num_key_value_heads=4)
    m._fork_limit("generate_beam", 16)
    for n in (0, 17):
        with pytest.raises(KvzError, match="at most 16 branches"):
            m._fork_limit("generate_beam", n)


def test_check_base_is_what_fork_asks():
    """What ``generate_beam`` / ``generate_samples`` ask before they append the query's rows to the base: ``fork()``'s own refusals."""
    from kvzip_amd.ops import KvzError
    with pytest.raises(KvzError, match="needs a pruned EvictCache in the slack layout"):
        ForkedCache.check_base(types.SimpleNamespace(pruned=True, info={"flatten": True}, layout="slack"), 2)
    with pytest.raises(KvzError, match="needs a pruned"):
        ForkedCache(types.SimpleNamespace(), 2)
    assert ForkedCache._closed is False and ForkedCache.__new__(ForkedCache)._closed is False
