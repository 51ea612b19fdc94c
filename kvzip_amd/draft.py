"""Drafting and acceptance for speculative decoding on a pruned cache (``ModelKVzip.generate_speculative``).

No reference counterpart: the reference decodes one token per forward pass.  The drafter here is the cheapest there is - prompt
lookup: long-context answers quote the context, so the tokens that followed the latest earlier occurrence of the last few tokens are
proposed as the next ones.  It needs no second model; any callable ``draft(history_ids, n) -> 1-D ids`` can take its place.

The tree form (``generate_speculative(tree=True)``) removes the bet on ONE earlier occurrence: ``lookup_tree`` proposes the
continuations behind several occurrences as a trie, ``accept_tree_greedy`` walks it along the model's argmax.  Any callable
``draft(history_ids, n) -> (ids, parents)`` can take its place there.
"""
from __future__ import annotations

import torch


def lookup_draft(history: torch.Tensor, n: int, ngram_max: int = 3, ngram_min: int = 1) -> torch.Tensor:
    """Up to ``n`` ids that continue ``history`` (1-D ids, any device) by prompt lookup: for the longest n-gram length in
    ``[ngram_min, ngram_max]`` whose last ``g`` ids occur BEFORE the end of ``history`` as well, the ids that followed the latest
    such occurrence (fewer than ``n`` where the continuation runs into the end); an empty tensor when there is none.  torch ops only
    (unfold / compare over all positions at once), one host synchronisation per tried length."""
    history = history.reshape(-1)
    L = history.shape[0]
    empty = history[:0]
    if n <= 0:
        return empty
    for g in range(min(int(ngram_max), L - 1), max(int(ngram_min), 1) - 1, -1):
        windows = history[:L - 1].unfold(0, g, 1)                 # starts 0 .. L-1-g: every occurrence has an id behind it
        hit = (windows == history[L - g:]).all(-1)
        pos = torch.where(hit, torch.arange(hit.shape[0], device=history.device), -1).max()
        i = int(pos)
        if i >= 0:
            return history[i + g:i + g + n]
    return empty


def accept_greedy(draft_ids: torch.Tensor, argmax_ids: torch.Tensor) -> int:
    """Number of leading draft tokens the model agrees with under greedy decoding: ``draft_ids[i]`` is accepted while it equals
    ``argmax_ids[i]``, the model's argmax at the position BEFORE it (``argmax_ids`` has at least as many entries as the draft: one per
    position of the verify pass)."""
    draft_ids, argmax_ids = draft_ids.reshape(-1), argmax_ids.reshape(-1)
    d = draft_ids.shape[0]
    if d == 0:
        return 0
    assert argmax_ids.shape[0] >= d
    same = (draft_ids == argmax_ids[:d].to(draft_ids.device)).to(torch.int64)
    return int(same.cumprod(0).sum())


def lookup_tree(history: torch.Tensor, n: int, ngram_max: int = 3, ngram_min: int = 1, max_branches: int = 4):
    """Up to ``n`` nodes that continue ``history`` as a TREE, by prompt lookup: ``(ids [m], parents [m])``, m <= n, the nodes BEHIND
    the root.  ``parents`` (a list of ints) indexes the full node list of the verify step, in which node 0 is the last token of
    ``history`` and ``ids[i]`` is node i + 1; a first-level node has parent 0.  For the longest n-gram length in ``[ngram_min,
    ngram_max]`` that occurs before the end of ``history`` as well, the continuations behind up to ``max_branches`` occurrences,
    latest first, are merged into a trie (equal prefixes share nodes).  The budget ``n`` is dealt breadth-first over the
    occurrences - depth 1 of every occurrence, then depth 2, ... - and a token that is already in the trie costs nothing.  Node order
    is depth-first with the latest occurrence's child first, so parents precede children and a tree with one occurrence is exactly
    ``lookup_draft``'s chain.  Deterministic; torch ops over all positions at once, one host synchronisation per tried length and one
    for the continuations."""
    history = history.reshape(-1)
    L = history.shape[0]
    if n <= 0 or max_branches <= 0:
        return history[:0], []
    for g in range(min(int(ngram_max), L - 1), max(int(ngram_min), 1) - 1, -1):
        windows = history[:L - 1].unfold(0, g, 1)                 # starts 0 .. L-1-g: every occurrence has an id behind it
        hit = (windows == history[L - g:]).all(-1)
        starts = torch.nonzero(hit).reshape(-1)
        if starts.shape[0] == 0:
            continue
        starts = starts.flip(0)[:int(max_branches)]               # latest first
        at = (starts + g)[:, None] + torch.arange(n, device=history.device)[None]
        cont = history[at.clamp(max=L - 1)].tolist()              # [occurrences][n]; entries at or beyond L are cut below
        avail = [min(n, L - int(a)) for a in (starts + g).tolist()]
        # the trie: node 0 is the root; children in the order the occurrences first asked for them
        tok, par, kids = [None], [-1], [[]]
        where = [0] * len(cont)                                   # node each occurrence has reached
        budget = n
        for d in range(n):
            for o, c in enumerate(cont):
                if d >= avail[o] or where[o] < 0:
                    continue
                nxt = next((k for k in kids[where[o]] if tok[k] == c[d]), None)
                if nxt is None:
                    if budget == 0:
                        where[o] = -1                             # (this occurrence goes no deeper)
                        continue
                    budget -= 1
                    nxt = len(tok)
                    tok.append(c[d]); par.append(where[o]); kids.append([])
                    kids[where[o]].append(nxt)
                where[o] = nxt
            if budget == 0:
                break
        ids, parents, number, stack = [], [], {0: 0}, list(reversed(kids[0]))
        while stack:                                              # depth-first, first child first
            k = stack.pop()
            number[k] = len(ids) + 1
            ids.append(tok[k]); parents.append(number[par[k]])
            stack += reversed(kids[k])
        return torch.tensor(ids, dtype=history.dtype, device=history.device), parents
    return history[:0], []


def accept_tree_greedy(ids, parents, argmax_ids) -> list:
    """The accepted path of a tree verify step under greedy decoding, as node indices including the root 0: from node 0 on, the
    child of node i whose id equals ``argmax_ids[i]`` (the model's argmax AT node i) is accepted, until a node has no such child.
    ``ids [m]`` / ``parents [m]`` describe the nodes behind the root as ``lookup_tree`` returns them (``ids[i]`` is node i + 1);
    ``argmax_ids`` has one entry per node, m + 1.  The path ascends (parents precede children)."""
    ids = ids.reshape(-1).tolist() if isinstance(ids, torch.Tensor) else [int(x) for x in ids]
    parents = parents.reshape(-1).tolist() if isinstance(parents, torch.Tensor) else [int(x) for x in parents]
    argmax = argmax_ids.reshape(-1).tolist() if isinstance(argmax_ids, torch.Tensor) else [int(x) for x in argmax_ids]
    assert len(parents) == len(ids) and len(argmax) >= len(ids) + 1
    path, cur = [0], 0
    while True:
        nxt = next((i + 1 for i in range(len(ids)) if parents[i] == cur and ids[i] == argmax[cur]), None)
        if nxt is None:
            return path
        path.append(nxt)
        cur = nxt
