"""Drafting and acceptance for speculative decoding on a pruned cache (``ModelKVzip.generate_speculative``).

No reference counterpart: the reference decodes one token per forward pass.  The drafter here is the cheapest there is - prompt
lookup: long-context answers quote the context, so the tokens that followed the latest earlier occurrence of the last few tokens are
proposed as the next ones.  It needs no second model; any callable ``draft(history_ids, n) -> 1-D ids`` can take its place.
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
