"""Tensor-level wrappers over the C ABI: torch is used for device memory and streams only.

Every function takes CUDA(=HIP) tensors, passes raw ``data_ptr()`` values plus the current HIP stream to
``libkvzip_hip.so`` and returns torch tensors that it allocated.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import math
import threading
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import KVZ_BF16, KVZ_F16, KvzError  # noqa: F401
from ._lib import check as _check

COMPACT_TILE = 1024


def _dtype_code(dtype: torch.dtype) -> int:
    if dtype == torch.float16:
        return KVZ_F16
    if dtype == torch.bfloat16:
        return KVZ_BF16
    raise KvzError(f"unsupported dtype {dtype}: the path computes in fp16 or bf16 "
                   "(reference csrc/csrc/static_switch.h:3-12)")


_tls = threading.local()  # .restore: device that was current before a call had to switch (given back by check() after the launch)


def _give_back_device() -> None:
    prev = getattr(_tls, "restore", None)
    if prev is not None:
        _tls.restore = None
        torch.cuda.set_device(prev)


def check(rc: int, who: str) -> None:
    """Raise on a non-zero return code; give the caller back the current device it had before the call (see ``_stream``)."""
    _give_back_device()
    _check(rc, who)


def _stream(t: torch.Tensor) -> int:
    """HIP stream handle for a launch on ``t``'s device.  The library launches on the CURRENT HIP device, so a tensor that
    lives on another GPU (a cache on cuda:1 while cuda:0 is current) makes its device current for the call; ``check`` - which
    follows every launch - switches back, so the caller's current device is what it was.  The pending switch is per host thread,
    and a switch that a failed call left behind (an exception between ``_stream`` and ``check``) is undone by the next call
    before it looks at the current device.  Every cache object and every call of this module works on ONE device (all tensors
    of a call must share it)."""
    if not t.is_cuda:
        raise KvzError("the HIP path needs device tensors (no CPU fallback)")
    _give_back_device()
    cur = torch.cuda.current_device()
    if t.device.index != cur:
        _tls.restore = cur
        torch.cuda.set_device(t.device)
    return raw_stream(t.device.index)


try:  # the raw handle of the current stream without building a torch.cuda.Stream object (4 us -> 0.3 us per launch)
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:  # pragma: no cover
    _raw_stream = None


def raw_stream(device_index: int) -> int:
    if _raw_stream is not None:
        return _raw_stream(device_index)
    return torch.cuda.current_stream(device_index).cuda_stream


def _same_device(*tensors) -> None:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise KvzError(f"all tensors of a call must live on one device (got {dev} and {t.device})")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# --------------------------------------------------------------------------------------------------
# a1  scoring
# --------------------------------------------------------------------------------------------------
def score_chunk(query_states: torch.Tensor, key_states: torch.Tensor, sink: int, start: int, end: int,
                out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                stream: Optional["torch.cuda.Stream"] = None) -> torch.Tensor:
    """KV importance score of one layer / one chunk (reference attention/score.py:36-65).

    query_states ``[1, H, q, D]``, key_states ``[1, Hkv, klen, D]`` (rows contiguous; the head stride may be
    larger than ``klen*D`` — views into a cache with slack are fine).  Returns ``[1, Hkv, end-start]``.
    ``stream``: launch there instead of on the current stream (``out`` and ``workspace`` must then be given: nothing is
    allocated on a foreign stream).
    """
    lib = _lib.load()
    bsz, H, q_len, D = query_states.shape
    _, Hkv, klen, _ = key_states.shape
    assert bsz == 1, "batch size is 1 on this path (reference attention/score.py:29)"
    assert H % Hkv == 0
    G = H // Hkv
    m = end - start
    assert m > 0 and sink >= 0 and start >= sink and end <= klen - q_len, (sink, start, end, klen, q_len)
    dt = _dtype_code(query_states.dtype)
    assert key_states.dtype == query_states.dtype
    assert query_states.stride(-1) == 1 and query_states.stride(-2) == D
    assert key_states.stride(-1) == 1 and key_states.stride(-2) == D
    assert stream is None or (out is not None and workspace is not None)
    _same_device(query_states, key_states, out, workspace)
    if out is None:
        out = torch.empty((1, Hkv, m), dtype=query_states.dtype, device=query_states.device)
    assert out.stride(-1) == 1 and out.shape[-1] == m
    need = lib.kvz_score_workspace_bytes(Hkv, G, q_len, m, sink)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=query_states.device)
    rc = lib.kvz_score_chunk(query_states.data_ptr(), query_states.stride(1), key_states.data_ptr(),
                             key_states.stride(1), klen, sink, start, end, q_len, Hkv, G, D, dt,
                             out.data_ptr(), out.stride(1), workspace.data_ptr(), workspace.numel(),
                             _stream(query_states) if stream is None else stream.cuda_stream)
    check(rc, "kvz_score_chunk")
    return out


# --------------------------------------------------------------------------------------------------
# a4 / a5  selection
# --------------------------------------------------------------------------------------------------
def select_workspace(device) -> torch.Tensor:
    """Scratch of the global-threshold selection (two radix histograms); cleared by the library call that fills it."""
    return torch.empty(_lib.load().kvz_select_workspace_bytes(), dtype=torch.uint8, device=device)


def select_threshold(score: torch.Tensor, ratio: float, row_len: Optional[int] = None, prehist: Optional[torch.Tensor] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Global-threshold selection (reference attention/score.py:88-102) — device side only.

    Returns ``(valid bool like score, thres f32[1] (device), kept i64[1] (device), row_counts i32[rows] or None)``.
    No host synchronisation happens here.  ``prehist``: a selection workspace that already holds the first histogram of exactly
    these scores (``kvz_score_finalize_log_hist``, see ``KVScore._finalize_log``): one streaming pass less.
    """
    lib = _lib.load()
    assert prehist is None or score.is_contiguous()
    score = score.contiguous()
    n = score.numel()
    dt = _dtype_code(score.dtype)
    dev = score.device
    valid = torch.empty(score.shape, dtype=torch.bool, device=dev)
    thres = torch.empty(1, dtype=torch.float32, device=dev)
    kept = torch.empty(1, dtype=torch.int64, device=dev)
    rows = None
    if row_len is not None:
        rows = torch.empty(n // row_len, dtype=torch.int32, device=dev)
    ws = prehist if prehist is not None else select_workspace(dev)
    fn = lib.kvz_select_threshold_prehist if (prehist is not None and ratio < 1) else lib.kvz_select_threshold
    rc = fn(score.data_ptr(), n, float(ratio), dt, valid.data_ptr(), row_len if row_len is not None else n, _ptr(rows),
            thres.data_ptr(), kept.data_ptr(), ws.data_ptr(), ws.numel(), _stream(score))
    check(rc, "kvz_select_threshold")
    return valid, thres, kept, rows


def select_heads(head_scores: torch.Tensor, N: int, ratio: float
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Head-level selection (reference model/wrapper.py:40-58 + attention/score.py:88-102) on the ``[L, Hkv]`` head scores
    themselves: the threshold of the N-fold expanded tensor is the head value of rank ``idx // N``.
    Returns ``(valid_heads bool [L, Hkv], thres f32[1], kept i64[1] (= N * kept heads), row_counts i32[L*Hkv])``."""
    lib = _lib.load()
    hs = head_scores.contiguous()
    rows = hs.numel()
    dev = hs.device
    valid = torch.empty(hs.shape, dtype=torch.bool, device=dev)
    thres = torch.empty(1, dtype=torch.float32, device=dev)
    kept = torch.empty(1, dtype=torch.int64, device=dev)
    counts = torch.empty(rows, dtype=torch.int32, device=dev)
    rc = lib.kvz_select_heads(hs.data_ptr(), rows, int(N), float(ratio), _dtype_code(hs.dtype), valid.data_ptr(),
                              counts.data_ptr(), thres.data_ptr(), kept.data_ptr(), _stream(hs))
    check(rc, "kvz_select_heads")
    return valid, thres, kept, counts


def rowmax(score: torch.Tensor) -> torch.Tensor:
    """Maximum over the last dim of 16-bit scores (head-score production, reference test.py:22-25)."""
    lib = _lib.load()
    score = score.contiguous()
    row_len = score.shape[-1]
    rows = score.numel() // row_len
    out = torch.empty(score.shape[:-1], dtype=score.dtype, device=score.device)
    rc = lib.kvz_rowmax16(score.data_ptr(), rows, row_len, _dtype_code(score.dtype), out.data_ptr(), _stream(score))
    check(rc, "kvz_rowmax16")
    return out


def select_topk_rows(score: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-row exact top-k over the last dim (reference attention/score.py:104-120)."""
    lib = _lib.load()
    score = score.contiguous()
    row_len = score.shape[-1]
    rows = score.numel() // row_len
    valid = torch.empty(score.shape, dtype=torch.bool, device=score.device)
    counts = torch.empty(rows, dtype=torch.int32, device=score.device)
    rc = lib.kvz_select_topk_rows(score.data_ptr(), rows, row_len, int(k), _dtype_code(score.dtype),
                                  valid.data_ptr(), counts.data_ptr(), _stream(score))
    check(rc, "kvz_select_topk_rows")
    return valid, counts


# --------------------------------------------------------------------------------------------------
# a8 / a9  compaction
# --------------------------------------------------------------------------------------------------
class CompactPlan:
    """Device-side result of ``kvz_compact_plan`` for all layers (reference attention/kvcache.py:168-185)."""

    def __init__(self, layers: int, Hkv: int, N: int, sink: int, klen: int, slack: int, device):
        self.layers, self.Hkv, self.N, self.sink, self.klen, self.slack = layers, Hkv, N, sink, klen, slack
        self.ntiles = (klen + COMPACT_TILE - 1) // COMPACT_TILE
        i32 = dict(dtype=torch.int32, device=device)
        # one allocation so that a single D2H copy brings all the metadata to the host
        meta = torch.empty(layers * Hkv * 2 + layers * (Hkv + 1) + layers, **i32)
        o = 0
        self.len_k = meta[o:o + layers * Hkv].view(layers, Hkv); o += layers * Hkv
        self.seg_start = meta[o:o + layers * Hkv].view(layers, Hkv); o += layers * Hkv
        self.cu_len_k = meta[o:o + layers * (Hkv + 1)].view(layers, Hkv + 1); o += layers * (Hkv + 1)
        self.max_len_k = meta[o:o + layers]
        self.meta = meta
        self.tile_base = torch.empty(layers * Hkv * self.ntiles, **i32)


def is_head_level(valid: torch.Tensor) -> bool:
    """True for a head-level mask: one value per (layer, head) broadcast over the context (stride 0 on the last dim)."""
    return valid.dim() >= 2 and valid.shape[-1] > 1 and valid.stride(-1) == 0


def compact_plan(valid: torch.Tensor, sink: int, klen: int, slack: int = 0) -> CompactPlan:
    """valid ``[L, 1, Hkv, N]`` (or ``[L, Hkv, N]``) bool -> per-layer varlen metadata on the device.
    A head-level mask (``[L, 1, Hkv, 1]`` expanded over N, stride 0) is planned from its L*Hkv bytes."""
    lib = _lib.load()
    L = valid.shape[0]
    Hkv, N = valid.shape[-2], valid.shape[-1]
    heads = is_head_level(valid)
    valid = valid[..., :1].contiguous() if heads else valid.contiguous()
    plan = CompactPlan(L, Hkv, N, sink, klen, slack, valid.device)
    fn = lib.kvz_compact_plan_heads if heads else lib.kvz_compact_plan
    rc = fn(valid.data_ptr(), L, Hkv, N, sink, klen, slack, plan.len_k.data_ptr(),
            plan.cu_len_k.data_ptr(), plan.seg_start.data_ptr(), plan.max_len_k.data_ptr(),
            plan.tile_base.data_ptr(), _stream(valid))
    check(rc, "kvz_compact_plan_heads" if heads else "kvz_compact_plan")
    plan.valid = valid
    plan.heads = heads
    return plan


def compact_layer(k: torch.Tensor, v: torch.Tensor, plan: CompactPlan, layer: int, total_rows: int
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Gather one layer: k, v ``[1, Hkv, klen, D]`` -> ``[total_rows, D]`` each (order preserving, head major)."""
    lib = _lib.load()
    _, Hkv, klen, D = k.shape
    assert klen == plan.klen and Hkv == plan.Hkv
    assert k.stride(-1) == 1 and k.stride(-2) == D and v.stride() == k.stride()
    k_out = torch.empty((total_rows, D), dtype=k.dtype, device=k.device)
    v_out = torch.empty((total_rows, D), dtype=v.dtype, device=v.device)
    if total_rows == 0:
        return k_out, v_out
    assert not getattr(plan, "heads", False), "head-level plans go through compact_layers"
    valid_l = plan.valid.view(plan.layers, Hkv, plan.N)[layer]
    tb = plan.tile_base.view(plan.layers, Hkv * plan.ntiles)[layer]
    rc = lib.kvz_compact_layer(k.data_ptr(), v.data_ptr(), k.stride(1), valid_l.data_ptr(), tb.data_ptr(),
                               plan.seg_start[layer].data_ptr(), Hkv, plan.N, plan.sink, klen, D,
                               k.element_size(), k_out.data_ptr(), v_out.data_ptr(), _stream(k))
    check(rc, "kvz_compact_layer")
    return k_out, v_out


def compact_layers(ks: Sequence[torch.Tensor], vs: Sequence[torch.Tensor], plan: CompactPlan,
                   totals: Sequence[int]) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
    """All layers in ONE launch (pointer tables).  ``totals[l]`` = rows to allocate for layer l."""
    lib = _lib.load()
    L = len(ks)
    assert L == plan.layers
    _, Hkv, klen, D = ks[0].shape
    dev = ks[0].device
    hs = ks[0].stride(1)
    for k, v in zip(ks, vs):
        assert k.shape == ks[0].shape and v.shape == ks[0].shape
        assert k.stride(-1) == 1 and k.stride(-2) == D and k.stride(1) == hs and v.stride() == k.stride()
    # (an all-evicted layer still gets a 1-row buffer so that its table entry is a valid pointer)
    k_outs = [torch.empty((max(int(t), 1), D), dtype=ks[0].dtype, device=dev)[:int(t)] for t in totals]
    v_outs = [torch.empty((max(int(t), 1), D), dtype=ks[0].dtype, device=dev)[:int(t)] for t in totals]
    table = torch.tensor([[t.data_ptr() for t in ks], [t.data_ptr() for t in vs],
                          [t.data_ptr() for t in k_outs], [t.data_ptr() for t in v_outs]],
                         dtype=torch.int64).to(dev, non_blocking=False)
    fn = lib.kvz_compact_layers_heads if getattr(plan, "heads", False) else lib.kvz_compact_layers
    rc = fn(table[0].data_ptr(), table[1].data_ptr(), hs, plan.valid.data_ptr(),
            plan.tile_base.data_ptr(), plan.seg_start.data_ptr(), L, Hkv, plan.N, plan.sink,
            klen, D, ks[0].element_size(), table[2].data_ptr(), table[3].data_ptr(),
            _stream(ks[0]))
    check(rc, "kvz_compact_layers")
    # keep the pointer table alive until the kernel has consumed it
    table.record_stream(torch.cuda.current_stream(dev))
    return k_outs, v_outs


# --------------------------------------------------------------------------------------------------
# tightening a pruned cache (include/kvzip_hip_tighten.h; no reference counterpart)
# --------------------------------------------------------------------------------------------------
def _mask_bytes(valid: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """(contiguous mask, tok1): a head-level mask (stride 0 over the context) goes down as its L*Hkv bytes, as in ``compact_plan``."""
    if is_head_level(valid):
        return valid[..., :1].contiguous(), 0
    return valid.contiguous(), 1


def mask_resurrects(new_valid: torch.Tensor, old_valid: torch.Tensor) -> torch.Tensor:
    """Number of positions ``new_valid`` keeps although ``old_valid`` evicted them, as a device int32 ``[1]`` (no host
    synchronisation).  Masks ``[L, 1, Hkv, N]`` / ``[L, Hkv, N]`` bool, token- or head-level each."""
    lib = _lib.load()
    assert new_valid.shape[-1] == old_valid.shape[-1] and new_valid.numel() == old_valid.numel()
    _same_device(new_valid, old_valid)
    N = new_valid.shape[-1]
    rows = new_valid.numel() // N
    nv, ntok1 = _mask_bytes(new_valid)
    ov, otok1 = _mask_bytes(old_valid)
    count = torch.empty(1, dtype=torch.int32, device=nv.device)
    rc = lib.kvz_mask_resurrects(nv.data_ptr(), ntok1, ov.data_ptr(), otok1, rows, N, count.data_ptr(), _stream(nv))
    check(rc, "kvz_mask_resurrects")
    return count


def recompact_layers(ks: Sequence[torch.Tensor], vs: Sequence[torch.Tensor], old_plan: CompactPlan, old_valid: torch.Tensor,
                     new_plan: CompactPlan, new_valid: torch.Tensor, totals: Sequence[int],
                     tail_rows: Optional[Sequence[int]] = None) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
    """Flat ``[rows, D]`` K, V of all layers in the layout of ``old_plan`` -> fresh buffers in the layout of ``new_plan``, ONE launch.
    ``new_valid`` must be a subset of ``old_valid`` (``mask_resurrects`` == 0).  ``totals[l]`` = rows to allocate for layer l;
    ``tail_rows[l]`` = rows appended behind every head of layer l after the old prune (they move behind the head's new rows)."""
    lib = _lib.load()
    L = len(ks)
    assert L == old_plan.layers == new_plan.layers and len(vs) == L and len(totals) == L
    for a in ("Hkv", "N", "sink", "klen", "ntiles"):
        assert getattr(old_plan, a) == getattr(new_plan, a), f"the two plans differ in {a}"
    D = ks[0].shape[-1]
    dev = ks[0].device
    for k, v in zip(ks, vs):
        assert k.dim() == 2 and k.shape == v.shape and k.shape[-1] == D and k.is_contiguous() and v.is_contiguous()
        assert k.dtype == ks[0].dtype and v.dtype == ks[0].dtype
    tail = None
    if tail_rows is not None and any(int(t) for t in tail_rows):
        assert len(tail_rows) == L
        if not 0 <= min(tail_rows) <= max(tail_rows) <= min(old_plan.slack, new_plan.slack):
            raise KvzError(f"recompact_layers: {max(tail_rows)} appended rows per head do not fit the slack "
                           f"({old_plan.slack} -> {new_plan.slack} rows)")
        tail = torch.tensor([int(t) for t in tail_rows], dtype=torch.int32).to(dev)
    ov, otok1 = _mask_bytes(old_valid)
    nv, ntok1 = _mask_bytes(new_valid)
    _same_device(ks[0], ov, nv, old_plan.tile_base, new_plan.tile_base)
    k_outs = [torch.empty((max(int(t), 1), D), dtype=ks[0].dtype, device=dev)[:int(t)] for t in totals]
    v_outs = [torch.empty((max(int(t), 1), D), dtype=ks[0].dtype, device=dev)[:int(t)] for t in totals]
    table = torch.tensor([[t.data_ptr() for t in ks], [t.data_ptr() for t in vs],
                          [t.data_ptr() for t in k_outs], [t.data_ptr() for t in v_outs]],
                         dtype=torch.int64).to(dev, non_blocking=False)
    old_seg, old_len = old_plan.seg_start.contiguous(), old_plan.len_k.contiguous()
    rc = lib.kvz_recompact_layers(table[0].data_ptr(), table[1].data_ptr(), ov.data_ptr(), otok1, old_plan.tile_base.data_ptr(),
                                  old_seg.data_ptr(), old_len.data_ptr(), nv.data_ptr(), ntok1, new_plan.tile_base.data_ptr(),
                                  new_plan.seg_start.data_ptr(), new_plan.len_k.data_ptr(), _ptr(tail), L, old_plan.Hkv, old_plan.N,
                                  old_plan.sink, old_plan.klen, D, ks[0].element_size(), table[2].data_ptr(), table[3].data_ptr(),
                                  _stream(ks[0]))
    check(rc, "kvz_recompact_layers")
    # keep the pointer table alive until the kernel has consumed it
    table.record_stream(torch.cuda.current_stream(dev))
    return k_outs, v_outs


# --------------------------------------------------------------------------------------------------
# a10 / a11  append
# --------------------------------------------------------------------------------------------------
def update_flatten_view(cache: torch.Tensor, state: torch.Tensor, headlens: torch.Tensor,
                        cu_headlens: torch.Tensor) -> torch.Tensor:
    """Drop-in for ``tiny_api_cuda.update_flatten_view`` (reference csrc/csrc/cuda_api.cu:68-111):
    same arguments, same dtype checks (-> RuntimeError), returns a fresh tensor."""
    lib = _lib.load()
    if headlens.dtype != torch.int32:
        raise KvzError("expected headlens to be int32")
    if cu_headlens.dtype != torch.int32:
        raise KvzError("expected cu_headlens to be int32")
    origin_len, dim = cache.shape
    head_num = headlens.shape[0]
    if state.shape[0] % head_num != 0:
        raise KvzError("state rows must be divisible by head count")
    t = state.shape[0] // head_num
    cache = cache.contiguous()
    state = state.contiguous()
    out = torch.empty((origin_len + head_num * t, dim), dtype=cache.dtype, device=cache.device)
    rc = lib.kvz_update_flatten_view(cache.data_ptr(), state.data_ptr(), headlens.data_ptr(),
                                     cu_headlens.data_ptr(), head_num, t, dim, cache.element_size(),
                                     out.data_ptr(), _stream(cache))
    check(rc, "kvz_update_flatten_view")
    return out


def append_inplace(k_cache: torch.Tensor, v_cache: torch.Tensor, k_state: torch.Tensor, v_state: torch.Tensor,
                   seg_start: torch.Tensor, base_len: torch.Tensor, len_offset: int = 0) -> None:
    """O(t) append of ``k_state/v_state [1, Hkv, t, D]`` after each head's current rows (slack layout)."""
    lib = _lib.load()
    _, Hkv, t, D = k_state.shape
    assert k_state.stride(-1) == 1 and v_state.stride(-1) == 1 and v_state.shape == k_state.shape
    rc = lib.kvz_append_inplace(k_cache.data_ptr(), v_cache.data_ptr(), k_state.data_ptr(), v_state.data_ptr(),
                                k_state.stride(1), k_state.stride(2), v_state.stride(1), v_state.stride(2),
                                seg_start.data_ptr(), base_len.data_ptr(), int(len_offset), Hkv, t, D,
                                k_cache.element_size(), _stream(k_cache))
    check(rc, "kvz_append_inplace")


# --------------------------------------------------------------------------------------------------
# a13  variable-length attention
# --------------------------------------------------------------------------------------------------
def attn_workspace(Hkv: int, G: int, q_len: int, D: int, device) -> torch.Tensor:
    """Scratch of the attention kernels: partial results of the key ranges (decode kernel) or of the key splits (multi-row kernel).
    No initialisation is required; it is zero-filled once anyway (a reserved counter region of the layout)."""
    need = _lib.load().kvz_varlen_attn_workspace_bytes(Hkv, G, q_len, D, 0)
    return torch.zeros(max(int(need), 16), dtype=torch.uint8, device=device)


def _meta_host(k_start_host, k_len_host, Hkv):
    """ctypes int32 array [starts ++ lens] for the kernel arguments, or None."""
    if k_start_host is None or k_len_host is None or Hkv > 64:
        return None
    import ctypes as C
    return (C.c_int32 * (2 * Hkv))(*k_start_host, *k_len_host)


def varlen_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, k_start: torch.Tensor, k_len: torch.Tensor,
                q_len: int, max_len_k: int, causal: bool = True, softmax_scale: Optional[float] = None,
                workspace: Optional[torch.Tensor] = None, k_len_offset: int = 0, meta_host=None,
                offset_dev: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q ``[Hkv*q_len, G, D]``; k, v ``[rows, D]`` (or ``[rows, 1, D]``); head h owns rows
    ``k_start[h] : k_start[h]+k_len[h]``.  Returns ``[Hkv*q_len, G, D]``.  ``meta_host``: ctypes array from
    ``_meta_host`` (the segments as the host knows them) or None; ``workspace`` from ``attn_workspace``."""
    lib = _lib.load()
    HQ, G, D = q.shape
    Hkv = HQ // q_len
    assert Hkv * q_len == HQ and k_start.shape[0] == Hkv and k_len.shape[0] == Hkv
    assert k_start.dtype == torch.int32 and k_len.dtype == torch.int32
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty_like(q)
    if workspace is None:  # (a caller-provided workspace is validated by the library itself: KVZ_EWORKSPACE)
        workspace = attn_workspace(Hkv, G, q_len, D, q.device)
    rc = lib.kvz_varlen_attn(q.data_ptr(), k.data_ptr(), v.data_ptr(), k_start.data_ptr(), k_len.data_ptr(),
                             int(k_len_offset), _ptr(offset_dev), meta_host, Hkv, G,
                             q_len, D, int(max_len_k), float(scale), 1 if causal else 0, _dtype_code(q.dtype),
                             out.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream(q))
    check(rc, "kvz_varlen_attn")
    return out


def varlen_attn_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_state: torch.Tensor,
                       v_state: torch.Tensor, k_start: torch.Tensor, k_len: torch.Tensor, k_len_offset: int, max_len_k: int,
                       softmax_scale: Optional[float] = None, workspace: Optional[torch.Tensor] = None,
                       meta_host=None, offset_dev: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decode step in one launch: append the new token's K, V (``[1, Hkv, 1, D]``, any head stride) to the per-head slack
    of the flat cache and attend ``q`` (``[Hkv, G, D]``) over ``k_len + k_len_offset + 1`` keys.  ``k_len_offset`` counts the
    tokens appended BEFORE this call.  Bit-identical to ``append_inplace`` followed by ``varlen_attn``."""
    lib = _lib.load()
    Hkv, G, D = q.shape
    assert k_state.shape[-3] == Hkv and k_state.shape[-2] == 1 and v_state.shape[-2] == 1
    assert k_state.stride(-1) == 1 and v_state.stride(-1) == 1 and q.is_contiguous()
    assert k_start.dtype == torch.int32 and k_len.dtype == torch.int32
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty_like(q)
    if workspace is None:
        workspace = attn_workspace(Hkv, G, 1, D, q.device)
    rc = lib.kvz_varlen_attn_append(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_state.data_ptr(),
                                    v_state.data_ptr(), k_state.stride(-3), v_state.stride(-3), k_start.data_ptr(),
                                    k_len.data_ptr(), int(k_len_offset), _ptr(offset_dev), meta_host, Hkv, G, D, int(max_len_k), float(scale),
                                    _dtype_code(q.dtype), out.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream(q))
    check(rc, "kvz_varlen_attn_append")
    return out


def flash_fwd(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, causal: bool = True,
              softmax_scale: Optional[float] = None, return_lse: bool = False):
    """Dense GQA attention ``[1, H, q, D] x [1, Hkv, k, D] -> [1, q, H, D]`` with the causal mask aligned bottom-right
    (reference attention/attn.py:75-89, flash-attn's dense kernel).  ``key`` / ``value`` may be views of the dense cache
    (any head stride, rows contiguous); nothing is copied.  ``return_lse``: also the fp32 row LSE ``[1, H, q]``."""
    lib = _lib.load()
    b, H, q_len, D = query.shape
    Hkv, klen = key.shape[1], key.shape[2]
    G = H // Hkv
    assert b == 1 and key.shape[0] == 1 and G * Hkv == H and value.shape == key.shape
    if query.stride(-1) != 1 or query.stride(1) % 8 or query.stride(2) % 8:
        query = query.contiguous()

    def rows(t):  # [1, Hkv, k, D] view -> usable as "[rows, D], head h starts at row h * step"
        return t.stride(-1) == 1 and t.stride(2) == D and t.stride(1) % D == 0
    if not (rows(key) and rows(value) and key.stride(1) == value.stride(1)):
        key, value = key.contiguous(), value.contiguous()
    step = key.stride(1) // D if Hkv > 1 else klen
    meta = _meta_host([h * step for h in range(Hkv)], [klen] * Hkv, Hkv)
    assert meta is not None, "flash_fwd: more than 64 KV heads"
    out = torch.empty(1, q_len, H, D, dtype=query.dtype, device=query.device)
    lse = torch.empty(1, Hkv, q_len, G, dtype=torch.float32, device=query.device) if return_lse else None
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    need = int(lib.kvz_flash_workspace_bytes(Hkv, G, q_len, D))  # > 0 only when there are too few query rows to fill the chip
    ws = torch.empty(need, dtype=torch.uint8, device=query.device) if need else None
    rc = lib.kvz_flash_fwd(query.data_ptr(), G * query.stride(1), query.stride(1), query.stride(2), key.data_ptr(),
                           value.data_ptr(), None, None, 0, meta, Hkv, G, q_len, D, float(scale), 1 if causal else 0,
                           _dtype_code(query.dtype), out.data_ptr(), G * D, D, H * D, _ptr(lse), _ptr(ws), need,
                           _stream(query))
    check(rc, "kvz_flash_fwd")
    if return_lse:
        return out, lse.permute(0, 1, 3, 2).reshape(1, H, q_len)
    return out


# --------------------------------------------------------------------------------------------------
# forked decode: B queries over one shared pruned cache (no reference counterpart: batch is 1 there)
# --------------------------------------------------------------------------------------------------
FORK_MAX_ROWS = 64      # query rows (branches x query heads per KV head) of one forked decode launch
FORK_MAX_BRANCHES = 16


def fork_attn_workspace(B: int, Hkv: int, G: int, D: int, device) -> torch.Tensor:
    """Scratch of ``fork_attn_append`` (partials of the shared key ranges and of the tails); no initialisation needed."""
    need = _lib.load().kvz_fork_attn_workspace_bytes(B, Hkv, G, D, 0)
    return torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)


def fork_attn_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_start: Optional[torch.Tensor],
                     k_len: Optional[torch.Tensor], k_len_offset: int, tail_k: torch.Tensor, tail_v: torch.Tensor,
                     tail_len: Sequence[int], k_new: torch.Tensor, v_new: torch.Tensor, softmax_scale: Optional[float] = None,
                     workspace: Optional[torch.Tensor] = None, meta_host=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One decode step of B branches over one shared flat cache (``kvz_fork_attn_append``).  q ``[B, Hkv, G, D]``; k_cache / v_cache
    ``[rows, D]`` (read only; head h owns rows ``k_start[h] : + k_len[h] + k_len_offset``, device arrays and / or ``meta_host``);
    tail_k / tail_v ``[B, Hkv, tail_cap, D]``; ``tail_len[b]`` rows in use (-1: inactive branch); k_new / v_new ``[B, Hkv, 1, D]``
    (any batch / head stride).  Writes the new rows to ``tail[b, :, tail_len[b]]`` and returns ``[B, Hkv, G, D]``."""
    import ctypes as C
    lib = _lib.load()
    B, Hkv, G, D = q.shape
    assert tail_k.shape == tail_v.shape and tail_k.shape[0] == B and tail_k.shape[1] == Hkv and tail_k.shape[3] == D
    assert q.is_contiguous() and tail_k.is_contiguous() and tail_v.is_contiguous() and k_cache.is_contiguous() and v_cache.is_contiguous()
    assert k_new.shape == (B, Hkv, 1, D) and v_new.shape == (B, Hkv, 1, D) and k_new.stride(-1) == 1 and v_new.stride(-1) == 1
    assert len(tail_len) == B
    assert (k_start is None) == (k_len is None) and (k_start is not None or meta_host is not None)
    assert k_start is None or (k_start.dtype == torch.int32 and k_len.dtype == torch.int32)
    _same_device(q, k_cache, v_cache, tail_k, tail_v, k_new, v_new, workspace, out)
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty_like(q)
    if workspace is None:
        workspace = fork_attn_workspace(B, Hkv, G, D, q.device)
    tl = (C.c_int32 * B)(*[int(x) for x in tail_len])
    rc = lib.kvz_fork_attn_append(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), _ptr(k_start), _ptr(k_len), int(k_len_offset),
                                  meta_host, tail_k.data_ptr(), tail_v.data_ptr(), tail_k.shape[2], tl, k_new.data_ptr(),
                                  v_new.data_ptr(), k_new.stride(0), k_new.stride(1), v_new.stride(0), v_new.stride(1), B, Hkv, G, D,
                                  float(scale), _dtype_code(q.dtype), out.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream(q))
    check(rc, "kvz_fork_attn_append")
    return out


def attn_merge_lse(o1: torch.Tensor, lse1: torch.Tensor, o2: torch.Tensor, lse2: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Merge two partial attention results over disjoint key sets by their natural-log LSEs (``kvz_attn_merge_lse``): o1, o2
    ``[..., D]`` 16-bit, lse1, lse2 fp32 of the leading shape (-inf: that side saw no key)."""
    lib = _lib.load()
    D = o1.shape[-1]
    rows = o1.numel() // D
    assert o2.shape == o1.shape and o1.is_contiguous() and o2.is_contiguous() and o1.dtype == o2.dtype
    assert lse1.numel() == rows and lse2.numel() == rows and lse1.dtype == torch.float32 and lse2.dtype == torch.float32
    assert lse1.is_contiguous() and lse2.is_contiguous()
    _same_device(o1, o2, lse1, lse2, out)
    if out is None:
        out = torch.empty_like(o1)
    rc = lib.kvz_attn_merge_lse(o1.data_ptr(), lse1.data_ptr(), o2.data_ptr(), lse2.data_ptr(), out.data_ptr(), rows, D,
                                _dtype_code(o1.dtype), _stream(o1))
    check(rc, "kvz_attn_merge_lse")
    return out


# --------------------------------------------------------------------------------------------------
# speculative decoding: one verify step of t consecutive positions on a pruned cache (no reference counterpart)
# --------------------------------------------------------------------------------------------------
SPEC_MAX_ROWS = 64      # query rows (positions x query heads per KV head) of one verify launch


def spec_attn_workspace(t: int, Hkv: int, G: int, D: int, device) -> torch.Tensor:
    """Scratch of ``spec_attn_append`` (partials of the key ranges and of the triangle); no initialisation needed."""
    need = _lib.load().kvz_spec_attn_workspace_bytes(t, Hkv, G, D)
    return torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)


def spec_attn_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_start: Optional[torch.Tensor],
                     k_len: Optional[torch.Tensor], k_len_offset: int, slack: int, k_new: torch.Tensor, v_new: torch.Tensor,
                     softmax_scale: Optional[float] = None, workspace: Optional[torch.Tensor] = None, meta_host=None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One verify step on a pruned slack-layout cache (``kvz_spec_attn_append``).  q ``[Hkv, t, G, D]``; k_cache / v_cache
    ``[rows, D]``, head h holding ``k_len[h] + k_len_offset`` rows from ``k_start[h]`` on (device arrays and / or ``meta_host``) with
    ``slack`` free rows laid out behind every segment; k_new / v_new ``[Hkv, t, D]`` (any head / position stride).  Appends the t rows
    behind every segment and returns ``[Hkv, t, G, D]``: position p attends to the old rows and to the new rows 0 .. p."""
    lib = _lib.load()
    Hkv, t, G, D = q.shape
    assert q.is_contiguous() and k_cache.is_contiguous() and v_cache.is_contiguous()
    assert k_new.shape == (Hkv, t, D) and v_new.shape == (Hkv, t, D) and k_new.stride(-1) == 1 and v_new.stride(-1) == 1
    assert (k_start is None) == (k_len is None) and (k_start is not None or meta_host is not None)
    assert k_start is None or (k_start.dtype == torch.int32 and k_len.dtype == torch.int32)
    _same_device(q, k_cache, v_cache, k_new, v_new, workspace, out)
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty_like(q)
    assert out.shape == q.shape and out.is_contiguous() and out.dtype == q.dtype
    if workspace is None:
        workspace = spec_attn_workspace(t, Hkv, G, D, q.device)
    rc = lib.kvz_spec_attn_append(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), _ptr(k_start), _ptr(k_len), int(k_len_offset),
                                  meta_host, int(slack), k_new.data_ptr(), v_new.data_ptr(), k_new.stride(0), k_new.stride(1),
                                  v_new.stride(0), v_new.stride(1), t, Hkv, G, D, float(scale), _dtype_code(q.dtype), out.data_ptr(),
                                  workspace.data_ptr(), workspace.numel(), _stream(q))
    check(rc, "kvz_spec_attn_append")
    return out


# --------------------------------------------------------------------------------------------------
# tree speculative decoding (include/kvzip_hip_tree.h): verify a tree of drafted nodes in one step, keep the accepted path
# --------------------------------------------------------------------------------------------------
TREE_MAX_NODES = 64     # nodes of one verify step: one bit each in an ancestor mask


def ancestor_masks(parents: Sequence[int]) -> list:
    """Ancestor masks of a tree given by its parent vector (``parents[0] = -1``, ``parents[i] < i``: topological order): entry p has
    bit j set iff node j is p itself or one of its ancestors.  Pure Python; at most ``TREE_MAX_NODES`` nodes."""
    parents = [int(x) for x in parents]
    t = len(parents)
    if t == 0:
        return []
    if t > TREE_MAX_NODES:
        raise KvzError(f"ancestor_masks: {t} nodes (at most {TREE_MAX_NODES}: one bit each)")
    if parents[0] != -1:
        raise KvzError(f"ancestor_masks: parents[0] = {parents[0]} (node 0 is the root: -1)")
    masks = [1]
    for i in range(1, t):
        if not 0 <= parents[i] < i:
            raise KvzError(f"ancestor_masks: parents[{i}] = {parents[i]} (a node continues an EARLIER node: 0 .. {i - 1})")
        masks.append(masks[parents[i]] | (1 << i))
    return masks


def mask_array(anc: Sequence[int]):
    """The ancestor masks as the ctypes uint64 array ``tree_attn_append`` hands to the library."""
    import ctypes as C
    return (C.c_uint64 * len(anc))(*[int(m) for m in anc])


def tree_attn_workspace(t: int, Hkv: int, G: int, D: int, device) -> torch.Tensor:
    """Scratch of ``tree_attn_append`` (the size of the chain verify call's); no initialisation needed."""
    need = _lib.load().kvz_tree_attn_workspace_bytes(t, Hkv, G, D)
    return torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)


def tree_attn_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_start: Optional[torch.Tensor],
                     k_len: Optional[torch.Tensor], k_len_offset: int, slack: int, k_new: torch.Tensor, v_new: torch.Tensor,
                     anc: Sequence[int], softmax_scale: Optional[float] = None, workspace: Optional[torch.Tensor] = None,
                     meta_host=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One verify step over a TREE of t nodes on a pruned slack-layout cache (``kvz_tree_attn_append``).  Shapes as
    ``spec_attn_append``; ``anc`` are the t ancestor masks (``ancestor_masks``, or ``mask_array`` of them).  Appends the t rows behind every segment in node
    order and returns ``[Hkv, t, G, D]``: node p attends to the old rows and to the new rows whose bit is set in ``anc[p]``."""
    import ctypes as C
    lib = _lib.load()
    Hkv, t, G, D = q.shape
    assert q.is_contiguous() and k_cache.is_contiguous() and v_cache.is_contiguous()
    assert k_new.shape == (Hkv, t, D) and v_new.shape == (Hkv, t, D) and k_new.stride(-1) == 1 and v_new.stride(-1) == 1
    assert (k_start is None) == (k_len is None) and (k_start is not None or meta_host is not None)
    assert k_start is None or (k_start.dtype == torch.int32 and k_len.dtype == torch.int32)
    assert len(anc) == t
    _same_device(q, k_cache, v_cache, k_new, v_new, workspace, out)
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty_like(q)
    assert out.shape == q.shape and out.is_contiguous() and out.dtype == q.dtype
    if workspace is None:
        workspace = tree_attn_workspace(t, Hkv, G, D, q.device)
    masks = anc if isinstance(anc, C.Array) else mask_array(anc)     # (a caller with one tree for all layers converts once)
    rc = lib.kvz_tree_attn_append(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), _ptr(k_start), _ptr(k_len), int(k_len_offset),
                                  meta_host, int(slack), k_new.data_ptr(), v_new.data_ptr(), k_new.stride(0), k_new.stride(1),
                                  v_new.stride(0), v_new.stride(1), t, Hkv, G, D, float(scale), _dtype_code(q.dtype), out.data_ptr(),
                                  workspace.data_ptr(), workspace.numel(), masks, _stream(q))
    check(rc, "kvz_tree_attn_append")
    return out


def tree_keep_path(k_caches: Sequence[torch.Tensor], v_caches: Sequence[torch.Tensor], row0: Sequence[int], path: Sequence[int],
                   t: int) -> None:
    """Keep the accepted path of the t node rows a tree verify step appended (``kvz_tree_keep_path``), all layers in one launch:
    k_caches / v_caches are the flat ``[rows, D]`` caches of the layers, ``row0[l * Hkv + h]`` the row of node 0's slot of (layer,
    head); row ``path[i]`` of every slot run ends up at slot i, in place.  An identity path launches nothing."""
    import ctypes as C
    lib = _lib.load()
    L = len(k_caches)
    assert L > 0 and len(v_caches) == L and len(row0) % L == 0
    Hkv = len(row0) // L
    D, dtype = k_caches[0].shape[-1], k_caches[0].dtype
    for k, v in zip(k_caches, v_caches):
        assert k.is_contiguous() and v.is_contiguous() and k.shape[-1] == D and v.shape[-1] == D and k.dtype == dtype and v.dtype == dtype
    _same_device(*k_caches, *v_caches)
    kp = (C.c_void_p * L)(*[k.data_ptr() for k in k_caches])
    vp = (C.c_void_p * L)(*[v.data_ptr() for v in v_caches])
    r0 = (C.c_int32 * len(row0))(*[int(x) for x in row0])
    n = len(path)
    ph = (C.c_int32 * max(n, 1))(*[int(x) for x in path])
    rc = lib.kvz_tree_keep_path(L, kp, vp, r0, ph, n, int(t), Hkv, D, _dtype_code(dtype), _stream(k_caches[0]))
    check(rc, "kvz_tree_keep_path")


# --------------------------------------------------------------------------------------------------
# attention over the dense cache through an index of kept rows (include/kvzip_hip_retain.h): RetainCache
# --------------------------------------------------------------------------------------------------
class RetainIndex:
    """Kept positions of every (layer, head) of a mask, packed back to back (``kvz_retain_index``), and what the host knows of them.
    ``idx`` int32 ``[max(total, 1)]`` on the device; ``starts[l][h]`` / ``counts[l][h]`` python ints; ``meta_host[l]`` the ctypes array
    ``starts ++ counts`` of layer l that the attention calls pass on by value; ``ctx_end`` = sink + N."""

    def __init__(self, idx: torch.Tensor, row_start: torch.Tensor, starts, counts, ctx_end: int):
        import ctypes as C
        self.idx, self.row_start, self.starts, self.counts, self.ctx_end = idx, row_start, starts, counts, int(ctx_end)
        self.total = sum(sum(c) for c in counts)
        Hkv = len(counts[0])
        self.meta_host = [(C.c_int32 * (2 * Hkv))(*s, *c) for s, c in zip(starts, counts)]


def retain_index(plan: CompactPlan, counts_host=None) -> RetainIndex:
    """Index of the positions in ``[0, sink + N)`` that the full mask of ``plan`` keeps (``compact_plan(valid, sink, sink + N)``: lengths
    and tile bases are the plan's).  One launch for all layers; ``counts_host`` (``[L][Hkv]``) spares the one copy of the lengths to the
    host when the caller has them already."""
    lib = _lib.load()
    assert plan.klen == plan.sink + plan.N, "the index covers the context: plan with klen = sink + N"
    L, Hkv = plan.layers, plan.Hkv
    counts = counts_host if counts_host is not None else plan.len_k.cpu().tolist()   # (one D2H copy per prune)
    starts, o = [], 0
    for l in range(L):
        row = []
        for h in range(Hkv):
            row.append(o)
            o += int(counts[l][h])
        starts.append(row)
    if o >= 2 ** 31:
        raise KvzError(f"retain index: {o} kept rows over all layers do not fit 32-bit entries")
    dev = plan.tile_base.device
    row_start = torch.tensor(starts, dtype=torch.int32).to(dev)
    idx = torch.empty(max(o, 1), dtype=torch.int32, device=dev)
    heads = getattr(plan, "heads", False)
    fn = lib.kvz_retain_index_heads if heads else lib.kvz_retain_index
    rc = fn(plan.valid.data_ptr(), L, Hkv, plan.N, plan.sink, plan.tile_base.data_ptr(), row_start.data_ptr(), idx.data_ptr(), o,
            _stream(idx))
    check(rc, "kvz_retain_index_heads" if heads else "kvz_retain_index")
    return RetainIndex(idx, row_start, starts, [[int(c) for c in r] for r in counts], plan.klen)


def retain_attn_workspace(Hkv: int, G: int, q_len: int, D: int, device) -> torch.Tensor:
    """Scratch of ``retain_attn`` / ``retain_attn_append`` (partials of the key ranges); no initialisation needed."""
    need = _lib.load().kvz_retain_attn_workspace_bytes(Hkv, G, q_len, D)
    return torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)


def _retain_store(k_store: torch.Tensor, v_store: torch.Tensor):
    """(Hkv, capacity, D, head stride) of a dense ``[1, Hkv, capacity, D]`` (or ``[Hkv, capacity, D]``) store pair."""
    Hkv, cap, D = k_store.shape[-3:]
    assert v_store.shape == k_store.shape and v_store.dtype == k_store.dtype
    assert k_store.stride(-1) == 1 and k_store.stride(-2) == D and v_store.stride()[-3:] == k_store.stride()[-3:]
    return Hkv, cap, D, k_store.stride(-3)


def retain_attn(q: torch.Tensor, k_store: torch.Tensor, v_store: torch.Tensor, idx: torch.Tensor, meta_host, ctx_end: int, fill: int,
                q_len: int, causal: bool = True, softmax_scale: Optional[float] = None, workspace: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q ``[Hkv*q_len, G, D]`` (row p*G + g of head h, as ``prepare`` lays them out) over the dense store ``[1, Hkv, capacity, D]`` of
    which ``fill`` rows per head are in use: head h attends to the positions ``idx[start_h : start_h + n_h]`` (``meta_host`` = ctypes
    int32 ``starts ++ counts``) and to the rows ``ctx_end .. fill - 1``.  Returns ``[Hkv*q_len, G, D]``: the bits of ``varlen_attn`` on
    the compacted copy of the same rows."""
    lib = _lib.load()
    HQ, G, D = q.shape
    Hkv, cap, Ds, hs = _retain_store(k_store, v_store)
    assert Hkv * q_len == HQ and Ds == D and q.is_contiguous() and idx.dtype == torch.int32 and idx.is_contiguous()
    _same_device(q, k_store, v_store, idx, workspace, out)
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty_like(q)
    if workspace is None:
        workspace = retain_attn_workspace(Hkv, G, q_len, D, q.device)
    rc = lib.kvz_retain_attn(q.data_ptr(), k_store.data_ptr(), v_store.data_ptr(), hs, cap, idx.data_ptr(), idx.numel(), meta_host,
                             int(ctx_end), int(fill), Hkv, G, q_len, D, float(scale), 1 if causal else 0, _dtype_code(q.dtype),
                             out.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream(q))
    check(rc, "kvz_retain_attn")
    return out


def retain_attn_append(q: torch.Tensor, k_store: torch.Tensor, v_store: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor,
                       idx: torch.Tensor, meta_host, ctx_end: int, fill: int, softmax_scale: Optional[float] = None,
                       workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decode step in one call: write the new token's K, V (``[1, Hkv, 1, D]``, any head stride) into row ``fill`` of every head of
    the dense store and attend q (``[Hkv, G, D]``) over the indexed positions and the rows ``ctx_end .. fill``.  Bit-identical to
    ``kvz_dense_append`` followed by ``retain_attn`` with ``fill + 1``."""
    lib = _lib.load()
    Hkv, G, D = q.shape
    Hs, cap, Ds, hs = _retain_store(k_store, v_store)
    assert Hs == Hkv and Ds == D and q.is_contiguous() and idx.dtype == torch.int32 and idx.is_contiguous()
    assert k_new.shape[-3] == Hkv and k_new.shape[-2] == 1 and v_new.shape[-2] == 1 and k_new.shape[-1] == D
    assert k_new.stride(-1) == 1 and v_new.stride(-1) == 1
    _same_device(q, k_store, v_store, k_new, v_new, idx, workspace, out)
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty_like(q)
    if workspace is None:
        workspace = retain_attn_workspace(Hkv, G, 1, D, q.device)
    rc = lib.kvz_retain_attn_append(q.data_ptr(), k_store.data_ptr(), v_store.data_ptr(), hs, cap, k_new.data_ptr(), v_new.data_ptr(),
                                    k_new.stride(-3), v_new.stride(-3), idx.data_ptr(), idx.numel(), meta_host, int(ctx_end), int(fill),
                                    Hkv, G, D, float(scale), _dtype_code(q.dtype), out.data_ptr(), workspace.data_ptr(),
                                    workspace.numel(), _stream(q))
    check(rc, "kvz_retain_attn_append")
    return out


def fork_prefill_tail(query: torch.Tensor, cu_q: Sequence[int], tail_k: torch.Tensor, tail_v: torch.Tensor, tail_len: Sequence[int],
                      k_new: torch.Tensor, v_new: torch.Tensor, o_shared: torch.Tensor, lse_shared: torch.Tensor,
                      softmax_scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
                      branches: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The branch-private part of a PACKED first step (``kvz_fork_prefill_tail``, include/kvzip_hip_prefill.h): the queries of B
    branches back to back, branch b owning positions ``cu_q[b] : cu_q[b + 1]`` (host list of B + 1, ``cu_q[0] = 0``; an empty branch
    takes no part).  query ``[1, H, T, D]``, k_new / v_new ``[1, Hkv, T, D]`` (any head / position stride, rows contiguous); tail_k /
    tail_v ``[B, Hkv, tail_cap, D]`` with ``tail_len[b]`` rows in use; ``(o_shared [Hkv, T, G, D], lse_shared [Hkv, T, G])`` the
    partial result over the shared segments (``flash_fwd_ragged(..., causal=False)``).  Appends every branch's rows to its tail,
    attends every position over its own branch's tail (bottom-right causal) and returns the merge with the shared partial,
    ``[Hkv, T, G, D]``; ``out`` may be ``o_shared``.  ``branches``: a permutation of ``range(B)`` when the packing does not name the
    branches in ascending order - the b-th run of positions then belongs to tail ``branches[b]`` (``tail_len`` stays indexed by tail)."""
    import ctypes as C
    lib = _lib.load()
    b1, H, T, D = query.shape
    B, Hkv = tail_k.shape[0], tail_k.shape[1]
    G = H // Hkv
    assert b1 == 1 and G * Hkv == H and len(cu_q) == B + 1 and len(tail_len) == B
    assert tail_k.shape == tail_v.shape and tail_k.shape[3] == D and tail_k.is_contiguous() and tail_v.is_contiguous()
    assert k_new.shape == (1, Hkv, T, D) and v_new.shape == (1, Hkv, T, D)
    assert o_shared.shape == (Hkv, T, G, D) and o_shared.is_contiguous() and o_shared.dtype == query.dtype
    assert lse_shared.shape == (Hkv, T, G) and lse_shared.is_contiguous() and lse_shared.dtype == torch.float32
    if int(cu_q[B]) != T:
        raise KvzError(f"fork_prefill_tail: cu_q ends at {int(cu_q[B])}, the packed query holds {T} positions")
    if query.stride(-1) != 1 or query.stride(1) % 8 or query.stride(2) % 8:
        query = query.contiguous()
    if k_new.stride(-1) != 1 or k_new.stride(1) % 8 or k_new.stride(2) % 8:
        k_new = k_new.contiguous()
    if v_new.stride(-1) != 1 or v_new.stride(1) % 8 or v_new.stride(2) % 8:
        v_new = v_new.contiguous()
    _same_device(query, tail_k, tail_v, k_new, v_new, o_shared, lse_shared, out)
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty_like(o_shared)
    assert out.shape == o_shared.shape and out.is_contiguous() and out.dtype == o_shared.dtype
    if T == 0:   # (nothing packed: nothing to launch - and an empty tensor has no address to hand over)
        return out
    need = int(lib.kvz_fork_prefill_workspace_bytes(T, B, Hkv, G, D))
    ws = torch.empty(need, dtype=torch.uint8, device=query.device) if need else None
    cu = (C.c_int32 * (B + 1))(*[int(x) for x in cu_q])
    tl = (C.c_int32 * B)(*[int(x) for x in tail_len])
    assert branches is None or len(branches) == B
    br = None if branches is None else (C.c_int32 * B)(*[int(x) for x in branches])
    rc = lib.kvz_fork_prefill_tail(query.data_ptr(), G * query.stride(1), query.stride(1), query.stride(2), cu, tail_k.data_ptr(),
                                   tail_v.data_ptr(), tail_k.shape[2], tl, k_new.data_ptr(), v_new.data_ptr(), k_new.stride(1),
                                   k_new.stride(2), v_new.stride(1), v_new.stride(2), o_shared.data_ptr(), lse_shared.data_ptr(),
                                   out.data_ptr(), br, B, Hkv, G, D, float(scale), _dtype_code(query.dtype), _ptr(ws), need,
                                   _stream(query))
    check(rc, "kvz_fork_prefill_tail")
    return out


def fork_branch_copy(tail_k_list: Sequence[torch.Tensor], tail_v_list: Sequence[torch.Tensor], pairs: Sequence[Tuple[int, int]],
                     rows: Sequence[int]) -> None:
    """Move tail rows between the branch slots of a fork, all layers in one launch (``kvz_fork_branch_copy``,
    include/kvzip_hip_branch.h).  tail_k_list / tail_v_list: per layer ``[B, Hkv, tail_cap, D]`` contiguous (the capacity may differ
    between layers); for every layer, pair ``(src, dst) = pairs[i]`` and head: ``tail[dst, h, :rows[i]] = tail[src, h, :rows[i]]``,
    K and V alike - the only bytes written.  Sources and destinations are disjoint sets and no destination appears twice (the library
    refuses anything else: the copy is in place)."""
    import ctypes as C
    lib = _lib.load()
    L, P = len(tail_k_list), len(pairs)
    assert L >= 1 and len(tail_v_list) == L and len(rows) == P
    B, Hkv, _, D = tail_k_list[0].shape
    for k, v in zip(tail_k_list, tail_v_list):
        assert k.shape == v.shape and k.shape[0] == B and k.shape[1] == Hkv and k.shape[3] == D and k.dtype == tail_k_list[0].dtype
        assert k.is_contiguous() and v.is_contiguous() and v.dtype == k.dtype
    _same_device(*tail_k_list, *tail_v_list)
    kp = (C.c_void_p * L)(*[k.data_ptr() for k in tail_k_list])
    vp = (C.c_void_p * L)(*[v.data_ptr() for v in tail_v_list])
    cap = (C.c_int32 * L)(*[k.shape[2] for k in tail_k_list])
    n = max(P, 1)
    src = (C.c_int32 * n)(*[int(s) for s, _ in pairs])
    dst = (C.c_int32 * n)(*[int(d) for _, d in pairs])
    rw = (C.c_int32 * n)(*[int(r) for r in rows])
    rc = lib.kvz_fork_branch_copy(kp, vp, cap, L, B, Hkv, D, tail_k_list[0].element_size(), src, dst, rw, P, _stream(tail_k_list[0]))
    check(rc, "kvz_fork_branch_copy")


# --------------------------------------------------------------------------------------------------
# batched decode: one token for several INDEPENDENT pruned caches (include/kvzip_hip_multi.h; no reference counterpart)
# --------------------------------------------------------------------------------------------------
MULTI_MAX_CACHES = 16       # caches of one batched decode launch
MULTI_MAX_SEGMENTS = 128    # caches x KV heads
MULTI_MAX_HEADS = 64
MULTI_MAX_GROUP = 64        # query heads per KV head


class MultiTable:
    """The segments of B slack-layout caches (one layer) as the host arrays ``kvz_multi_attn_append`` takes: made once per layout of
    the caches, so that a decode step builds nothing but its B offsets.  Holds ADDRESSES, not tensors: whoever keeps a table keeps
    the caches and makes a new one when a cache was re-laid out (``kvcache.CacheBatch``)."""

    def __init__(self, k_caches: Sequence[torch.Tensor], v_caches: Sequence[torch.Tensor], seg_starts: Sequence[Sequence[int]],
                 lens: Sequence[Sequence[int]], slacks: Sequence[int]):
        import ctypes as C
        B = len(k_caches)
        assert B >= 1 and len(v_caches) == B and len(seg_starts) == B and len(lens) == B and len(slacks) == B
        Hkv = len(seg_starts[0])
        assert all(len(s) == Hkv for s in seg_starts) and all(len(n) == Hkv for n in lens)
        _same_device(*k_caches, *v_caches)
        for k, v in zip(k_caches, v_caches):
            assert k.is_contiguous() and v.is_contiguous() and k.shape == v.shape and k.dtype == k_caches[0].dtype
            assert k.shape[-1] == k_caches[0].shape[-1]
        self.B, self.Hkv, self.D, self.dtype, self.device = B, Hkv, k_caches[0].shape[-1], k_caches[0].dtype, k_caches[0].device
        self.k_ptrs = (C.c_void_p * B)(*[k.data_ptr() for k in k_caches])
        self.v_ptrs = (C.c_void_p * B)(*[v.data_ptr() for v in v_caches])
        self.seg = (C.c_int32 * (B * Hkv))(*[int(x) for s in seg_starts for x in s])
        self.lens = (C.c_int32 * (B * Hkv))(*[int(x) for n in lens for x in n])
        self.slack = (C.c_int32 * B)(*[int(x) for x in slacks])


def multi_attn_workspace(B: int, Hkv: int, G: int, D: int, device) -> torch.Tensor:
    """Scratch of ``multi_attn_append`` (partials of the key ranges); no initialisation needed, no dependence on the key lengths."""
    need = _lib.load().kvz_multi_attn_workspace_bytes(B, Hkv, G, D)
    return torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)


def multi_attn_append(q: torch.Tensor, table: MultiTable, offsets: Sequence[int], k_new: torch.Tensor, v_new: torch.Tensor,
                      softmax_scale: Optional[float] = None, workspace: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One decode step of B independent caches in one launch (``kvz_multi_attn_append``).  q ``[B, Hkv, G, D]``; ``table`` the
    caches' segments; ``offsets[b]`` rows appended to cache b before this call (-1: inactive cache - nothing of it is read or
    written, its output rows are zero); k_new / v_new ``[B, Hkv, 1, D]`` (any batch / head stride).  Writes the new rows to row
    ``seg_start + len + offset`` of every head segment of every live cache and returns ``[B, Hkv, G, D]``."""
    import ctypes as C
    lib = _lib.load()
    B, Hkv, G, D = q.shape
    assert table.B == B and table.Hkv == Hkv and table.D == D and table.dtype == q.dtype and len(offsets) == B
    assert q.is_contiguous()
    assert k_new.shape == (B, Hkv, 1, D) and v_new.shape == (B, Hkv, 1, D) and k_new.stride(-1) == 1 and v_new.stride(-1) == 1
    _same_device(q, k_new, v_new, workspace, out)
    if q.device != table.device:
        raise KvzError(f"all tensors of a call must live on one device (got {q.device} and the caches on {table.device})")
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty_like(q)
    assert out.is_contiguous() and out.shape == q.shape
    if workspace is None:
        workspace = multi_attn_workspace(B, Hkv, G, D, q.device)
    off = (C.c_int32 * B)(*[int(x) for x in offsets])
    rc = lib.kvz_multi_attn_append(q.data_ptr(), table.k_ptrs, table.v_ptrs, table.seg, table.lens, table.slack, off, k_new.data_ptr(),
                                   v_new.data_ptr(), k_new.stride(0), k_new.stride(1), v_new.stride(0), v_new.stride(1), B, Hkv, G, D,
                                   float(scale), _dtype_code(q.dtype), out.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream(q))
    check(rc, "kvz_multi_attn_append")
    return out


def multi_prefill_workspace(T: int, B: int, Hkv: int, G: int, D: int, device) -> torch.Tensor:
    """Scratch of ``multi_prefill`` for T packed positions (partials of the work items); no initialisation needed, no dependence on
    the key lengths."""
    need = _lib.load().kvz_multi_prefill_workspace_bytes(T, B, Hkv, G, D)
    return torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)


def multi_prefill(query: torch.Tensor, cu_q: Sequence[int], table: MultiTable, offsets: Sequence[int], k_new: torch.Tensor,
                  v_new: torch.Tensor, softmax_scale: Optional[float] = None, workspace: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The PACKED first step of B independent caches (``kvz_multi_prefill``, include/kvzip_hip_multi_prefill.h): their queries back
    to back, cache b owning positions ``cu_q[b] : cu_q[b + 1]`` (host list of B + 1, ``cu_q[0] = 0``; a cache without positions takes
    no part: nothing of it is read or written).  query ``[1, H, T, D]``, k_new / v_new ``[1, Hkv, T, D]`` (any head / position
    stride, rows contiguous); ``table`` the caches' segments; ``offsets[b]`` rows appended to cache b before this call.  Writes every
    cache's new rows to rows ``seg_start + len + offset ...`` of its head segments, attends every position over its own cache's
    segment and its own run up to itself, and returns ``[Hkv, T, G, D]``."""
    import ctypes as C
    lib = _lib.load()
    b1, H, T, D = query.shape
    B, Hkv = table.B, table.Hkv
    G = H // Hkv
    assert b1 == 1 and G * Hkv == H and len(cu_q) == B + 1 and len(offsets) == B
    assert table.D == D and table.dtype == query.dtype
    assert k_new.shape == (1, Hkv, T, D) and v_new.shape == (1, Hkv, T, D)
    if int(cu_q[B]) != T:
        raise KvzError(f"multi_prefill: cu_q ends at {int(cu_q[B])}, the packed query holds {T} positions")
    if query.stride(-1) != 1 or query.stride(1) % 8 or query.stride(2) % 8:
        query = query.contiguous()
    if k_new.stride(-1) != 1 or k_new.stride(1) % 8 or k_new.stride(2) % 8:
        k_new = k_new.contiguous()
    if v_new.stride(-1) != 1 or v_new.stride(1) % 8 or v_new.stride(2) % 8:
        v_new = v_new.contiguous()
    _same_device(query, k_new, v_new, workspace, out)
    if query.device != table.device:
        raise KvzError(f"all tensors of a call must live on one device (got {query.device} and the caches on {table.device})")
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty((Hkv, T, G, D), dtype=query.dtype, device=query.device)
    assert out.shape == (Hkv, T, G, D) and out.is_contiguous() and out.dtype == query.dtype
    if T == 0:   # (nothing packed: nothing to launch - and an empty tensor has no address to hand over)
        return out
    if workspace is None:
        workspace = multi_prefill_workspace(T, B, Hkv, G, D, query.device)
    cu = (C.c_int32 * (B + 1))(*[int(x) for x in cu_q])
    off = (C.c_int32 * B)(*[int(x) for x in offsets])
    rc = lib.kvz_multi_prefill(query.data_ptr(), G * query.stride(1), query.stride(1), query.stride(2), cu, table.k_ptrs, table.v_ptrs,
                               table.seg, table.lens, table.slack, off, k_new.data_ptr(), v_new.data_ptr(), k_new.stride(1),
                               k_new.stride(2), v_new.stride(1), v_new.stride(2), B, Hkv, G, D, float(scale),
                               _dtype_code(query.dtype), out.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream(query))
    check(rc, "kvz_multi_prefill")
    return out


def flash_fwd_ragged(query: torch.Tensor, k_flat: torch.Tensor, v_flat: torch.Tensor, starts: Sequence[int], lens: Sequence[int],
                     causal: bool, softmax_scale: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The ragged form of ``flash_fwd``: query ``[1, H, q, D]`` over flat K, V ``[rows, D]`` in which KV head h owns rows
    ``starts[h] : starts[h] + lens[h]`` (host lists, at most 64 heads).  Returns ``(out [Hkv, q, G, D], lse [Hkv, q, G] fp32)``;
    rows that see no key have lse -inf."""
    lib = _lib.load()
    b, H, q_len, D = query.shape
    Hkv = len(starts)
    G = H // Hkv
    assert b == 1 and G * Hkv == H and len(lens) == Hkv
    assert k_flat.is_contiguous() and v_flat.is_contiguous() and k_flat.shape[-1] == D
    rows = k_flat.numel() // D
    assert all(0 <= s and n >= 0 and s + n <= rows for s, n in zip(starts, lens)), "a head segment runs past the buffer"
    if query.stride(-1) != 1 or query.stride(1) % 8 or query.stride(2) % 8:
        query = query.contiguous()
    meta = _meta_host(list(starts), list(lens), Hkv)
    assert meta is not None, "flash_fwd_ragged: more than 64 KV heads"
    _same_device(query, k_flat, v_flat)
    out = torch.empty(Hkv, q_len, G, D, dtype=query.dtype, device=query.device)
    lse = torch.empty(Hkv, q_len, G, dtype=torch.float32, device=query.device)
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    need = int(lib.kvz_flash_workspace_bytes(Hkv, G, q_len, D))
    ws = torch.empty(need, dtype=torch.uint8, device=query.device) if need else None
    rc = lib.kvz_flash_fwd(query.data_ptr(), G * query.stride(1), query.stride(1), query.stride(2), k_flat.data_ptr(),
                           v_flat.data_ptr(), None, None, 0, meta, Hkv, G, q_len, D, float(scale), 1 if causal else 0,
                           _dtype_code(query.dtype), out.data_ptr(), q_len * G * D, D, G * D, lse.data_ptr(), _ptr(ws), need,
                           _stream(query))
    check(rc, "kvz_flash_fwd")
    return out, lse


def flash_fwd_window(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, sink: int, start: int, end: int,
                     stats: torch.Tensor, softmax_scale: Optional[float] = None) -> Optional[torch.Tensor]:
    """The dense causal forward of a scoring pass (``flash_fwd``) that also writes the row statistics of ``KVScore._get_score`` for the
    window ``sink ++ [start, end) ++ last q_len keys`` into ``stats`` (``[Hkv, stride, 2]`` fp32: (m_r, l'_r), row ``g*q_len + i``)
    from its own QK^T tiles.  Returns ``[1, q, H, D]``, or None when the 32-row kernel does not take the shape (the caller then
    scores with the two-pass kernels)."""
    lib = _lib.load()
    b, H, q_len, D = query.shape
    Hkv, klen = key.shape[1], key.shape[2]
    G = H // Hkv
    if (b != 1 or D != 128 or query.stride(-1) != 1 or query.stride(1) % 8 or query.stride(2) % 8 or key.stride(-1) != 1
            or key.stride(2) != D or key.stride(1) % D or value.stride(-1) != 1 or value.stride(2) != D or key.stride(1) != value.stride(1)):
        return None
    step = key.stride(1) // D if Hkv > 1 else klen
    meta = _meta_host([h * step for h in range(Hkv)], [klen] * Hkv, Hkv)
    if meta is None:
        return None
    out = torch.empty(1, q_len, H, D, dtype=query.dtype, device=query.device)
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    rc = lib.kvz_flash_fwd_window(query.data_ptr(), G * query.stride(1), query.stride(1), query.stride(2), key.data_ptr(),
                                  value.data_ptr(), meta, Hkv, G, q_len, D, float(scale), _dtype_code(query.dtype), out.data_ptr(),
                                  G * D, D, H * D, int(sink), int(start), int(end), stats.data_ptr(), stats.stride(0) // 2, _stream(query))
    if rc == -4:  # KVZ_EUNSUPPORTED: not a shape of the 32-row kernel
        check(0, "kvz_flash_fwd_window")
        return None
    check(rc, "kvz_flash_fwd_window")
    return out


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p=0.0,
                           softmax_scale=None, causal=False, seqused_k=None):
    """Call-compatible stand-in for the reference's use of ``flash_attn.flash_attn_varlen_func``
    (reference attention/attn.py:61-71): every "sequence" is one KV head with ``nheads_k = 1``."""
    assert dropout_p == 0.0
    Hkv = cu_seqlens_k.shape[0] - 1
    q_len = int(max_seqlen_q)
    k2 = k.view(-1, k.shape[-1])
    v2 = v.view(-1, v.shape[-1])
    k_start = cu_seqlens_k[:-1].contiguous()
    k_len = (cu_seqlens_k[1:] - cu_seqlens_k[:-1]).contiguous() if seqused_k is None else seqused_k
    assert q.shape[0] == Hkv * q_len
    return varlen_attn(q, k2, v2, k_start, k_len, q_len, int(max_seqlen_k), causal=causal,
                       softmax_scale=softmax_scale)
