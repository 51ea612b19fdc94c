"""KV caches with eviction — host-side mirror of the reference's ``EvictCache`` / ``RetainCache``
(reference attention/kvcache.py:14-347): same constructor, hooks (``update / _get_score / prepare``), user
calls (``prune / slice / init_score / get_seq_length / _mem``) and attributes; the data path runs in the
HIP kernels of ``include/kvzip_hip.h``.

MI355X-first storage (sized for 288 GB of HBM3E):
  * before pruning every layer owns ONE ``[1, Hkv, capacity, D]`` buffer; ``update`` writes the new rows in
    place (the reference re-allocates with ``torch.cat`` on every call, kvcache.py:75-78) and
    ``key_cache[l]`` is a view of the filled part;
  * ``prune`` compacts all layers in one launch into head-major ragged buffers; with ``layout="slack"``
    (default) every head segment is followed by ``slack`` free rows so that appending the query / generated
    tokens is O(t) and ``slice`` is O(1) (the reference rebuilds the whole flattened cache per layer and
    token through ``update_flatten_view``, kvcache.py:57-73); ``layout="packed"`` reproduces the reference's
    packed ``cu_len_k`` layout and its out-of-place append bit for bit.
"""
from __future__ import annotations

import contextlib
import copy
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .score import KVScore


def _model_props(model, device, dtype):
    cfg = model.config if hasattr(model, "config") else model
    if device is None or dtype is None:
        p = next(model.parameters())
        device = p.device if device is None else device
        dtype = p.dtype if dtype is None else dtype
    return cfg, torch.device(device), dtype


class _CacheBase(KVScore):
    """State shared by EvictCache and RetainCache (reference kvcache.py:18-39 / :222-242)."""

    def __init__(self, model, evict_range: Tuple[int, int], device=None, dtype=None, reserve: int = 4096):
        KVScore.__init__(self)
        cfg, self.device, self.dtype = _model_props(model, device, dtype)
        self.n_layers = cfg.num_hidden_layers
        self.n_heads = cfg.num_attention_heads
        self.n_heads_kv = cfg.num_key_value_heads
        self.n_group_kv = self.n_heads // self.n_heads_kv

        self.start_idx, self.end_idx = evict_range
        self.ctx_len = self.end_idx - self.start_idx
        self.sink = self.start_idx  # retain initial KV pairs for system prompts
        self.prefill_ids = None
        self.ctx_ids = None

        self.get_score = False  # indicator for KV scoring
        self.pruned = False     # whether KV cache is pruned or not
        self.valid = None
        self.valid_pad = torch.ones((1, self.n_heads_kv, self.start_idx), dtype=torch.bool, device=self.device)

        self.key_cache: List[torch.Tensor] = []
        self.value_cache: List[torch.Tensor] = []
        self._seen_tokens = 0
        self._store_k: List[torch.Tensor] = []   # [1, Hkv, capacity, D] per layer (pre-prune storage)
        self._store_v: List[torch.Tensor] = []
        self._fill: List[int] = []               # rows in use per layer
        self._reserve = int(reserve)
        self._views = {}                         # (layer, rows) -> (key view, value view, storage) of the dense cache
        self._pend_app = None                    # append left by update() for the fused update + score call of _get_score
        # scoring pass: update() leaves its append to the _get_score() call that follows it (attention/attn.py:44-54) and the two
        # become ONE library call.  Between the two calls the returned K,V views do not hold the new rows yet, so this is opt-in:
        # kvzip_amd.attn (the forward pass this package owns) and ModelKVzip.scoring switch it on
        self.fuse_update_score = False

    # -- dense (pre-prune) storage --------------------------------------------------------------
    def _dense_append(self, layer_idx: int, key_states: torch.Tensor, value_states: torch.Tensor):
        if key_states.is_cuda and key_states.device.index != self.device.index and self.device.index is not None:
            raise ops.KvzError(f"layer {layer_idx} lives on {key_states.device}, the cache on {self.device}: a cache object (its streams, "
                               "events and workspaces) works on ONE device - load the model on one GPU (one context per GPU is the "
                               "multi-GPU scheme, kvzip_amd/dist.py)")
        self._flush_append()
        t = key_states.shape[-2]
        if len(self._store_k) <= layer_idx:
            _, Hkv, _, D = key_states.shape
            cap = t + self._reserve
            self._store_k.append(torch.empty((1, Hkv, cap, D), dtype=key_states.dtype, device=key_states.device))
            self._store_v.append(torch.empty((1, Hkv, cap, D), dtype=value_states.dtype, device=value_states.device))
            self._fill.append(0)
            self.key_cache.append(None)
            self.value_cache.append(None)
        f = self._fill[layer_idx]
        sk, sv = self._dense_grow(layer_idx, f + t)
        fast = key_states.is_cuda and key_states.stride(-1) == 1 and value_states.stride(-1) == 1
        if fast and self.get_score and not self.pruned and self.fuse_update_score and self.score_deferred:
            # scoring pass: _get_score of this layer follows (attention/attn.py:44-54) and issues the append together with the
            # scoring kernels in ONE library call (kvz_update_score_async_log); anything else that touches the cache flushes first
            self._pend_app = (layer_idx, key_states, value_states, f)
        elif fast:
            # the previous (asynchronous) scoring call of this layer read the rows that are about to be overwritten
            if self._pending:
                self._wait_score(layer_idx)
            # one launch for K and V (strided sources accepted), scalars only: rows f .. f+t of every head
            lib = ops._lib.load()
            rc = lib.kvz_dense_append(sk.data_ptr(), sv.data_ptr(), sk.stride(1), f, key_states.data_ptr(), value_states.data_ptr(),
                                      key_states.stride(1), key_states.stride(2), value_states.stride(1), value_states.stride(2),
                                      sk.shape[1], t, sk.shape[3], sk.element_size(), ops._stream(sk))
            ops.check(rc, "kvz_dense_append")
        else:
            if self._pending:
                self._wait_score(layer_idx)
            sk[:, :, f:f + t].copy_(key_states)
            sv[:, :, f:f + t].copy_(value_states)
        self._dense_commit(layer_idx, f + t)

    def _dense_grow(self, layer_idx: int, need: int):
        """The layer's stores with room for ``need`` rows per head (amortised growth: the filled rows move to a larger buffer)."""
        f = self._fill[layer_idx]
        sk, sv = self._store_k[layer_idx], self._store_v[layer_idx]
        cap = sk.shape[2]
        if need > cap:
            self._wait_score(finalize=False)  # (scoring calls in flight read the storage that is being replaced)
            new_cap = max(2 * cap, need + self._reserve)
            for store in (self._store_k, self._store_v):
                old = store[layer_idx]
                new = torch.empty((1, old.shape[1], new_cap, old.shape[3]), dtype=old.dtype, device=old.device)
                new[:, :, :f].copy_(old[:, :, :f])
                store[layer_idx] = new
            sk, sv = self._store_k[layer_idx], self._store_v[layer_idx]
            self._views.clear()
        return sk, sv

    def _dense_commit(self, layer_idx: int, rows: int):
        """``rows`` rows per head of the layer are in use: the fill count and the ``key_cache`` / ``value_cache`` views."""
        sk, sv = self._store_k[layer_idx], self._store_v[layer_idx]
        self._fill[layer_idx] = rows
        # views of the filled part: the same lengths come back chunk after chunk (update ... slice), so they are cached
        vw = self._views.get((layer_idx, rows))
        if vw is None or vw[2] is not sk:
            vw = self._views[(layer_idx, rows)] = (sk[:, :, :rows], sv[:, :, :rows], sk)
            if len(self._views) > 16 * max(1, self.n_layers):
                self._views.clear()
        self.key_cache[layer_idx], self.value_cache[layer_idx] = vw[0], vw[1]

    def _flush_append(self):
        """Issue an append that update() left for _get_score (nothing else may see the cache without its rows)."""
        p = self._pend_app
        if p is None:
            return
        self._pend_app = None
        layer_idx, key_states, value_states, f = p
        if self._pending:
            self._wait_score(layer_idx)
        sk, sv = self._store_k[layer_idx], self._store_v[layer_idx]
        lib = ops._lib.load()
        rc = lib.kvz_dense_append(sk.data_ptr(), sv.data_ptr(), sk.stride(1), f, key_states.data_ptr(), value_states.data_ptr(),
                                  key_states.stride(1), key_states.stride(2), value_states.stride(1), value_states.stride(2),
                                  sk.shape[1], key_states.shape[-2], sk.shape[3], sk.element_size(), ops._stream(sk))
        ops.check(rc, "kvz_dense_append")

    def _dense_meta(self, cap: int, device):
        """(segment starts h*cap, zeros) int32 [Hkv] for the dense append launch, cached per capacity."""
        m = getattr(self, "_dense_meta_cache", None)
        if m is None or m[0] != cap:
            seg = torch.arange(self.n_heads_kv, dtype=torch.int32, device=device) * cap
            m = (cap, seg, torch.zeros(self.n_heads_kv, dtype=torch.int32, device=device))
            self._dense_meta_cache = m
        return m[1], m[2]

    def adopt_dense(self, store_k: List[torch.Tensor], store_v: List[torch.Tensor], filled: int):
        """Wrap already prefilled per-layer ``[1, Hkv, capacity, D]`` buffers without copying (e.g. the KV a
        serving engine prefilled elsewhere); ``filled`` rows are in use."""
        self._flush_append()
        self._wait_score(finalize=False)  # scoring calls still in flight read the storage that is being replaced
        self._views.clear()
        self._store_k, self._store_v = list(store_k), list(store_v)
        self._fill = [filled for _ in store_k]
        self.key_cache = [k[:, :, :filled] for k in self._store_k]
        self.value_cache = [v[:, :, :filled] for v in self._store_v]
        self._seen_tokens = filled

    def _dense_slice(self, seen_token_prev: int):
        self._flush_append()
        for l in range(len(self._store_k)):
            self._fill[l] = seen_token_prev
            self.key_cache[l] = self._store_k[l][:, :, :seen_token_prev]
            self.value_cache[l] = self._store_v[l][:, :, :seen_token_prev]

    def __del__(self):
        # asynchronous scoring reads the cache storage, the score buffer and the workspaces from side streams: order the
        # current stream behind it before the caching allocator may hand that memory to somebody else
        try:
            self._pend_app = None
            self._wait_score(finalize=False)
        except Exception:
            pass
        self._release_async()

    # reference: kvcache.py:108-112
    def get_seq_length(self, layer_idx: Optional[int] = 0) -> int:
        if len(self.key_cache) <= layer_idx:
            return 0
        return self._seen_tokens

    # reference: kvcache.py:140-150
    def _get_valid(self, layer_idx: int, n_seq: int) -> torch.Tensor:
        """full mask ``[1, Hkv, n_seq]`` = ones(sink) ++ valid[layer] ++ ones(rest)  (debug / interop helper; the
        kernels derive it on the fly)."""
        valid = torch.cat([self.valid_pad, self.valid[layer_idx]], dim=-1)
        size = list(valid.shape)
        size[-1] = n_seq - valid.shape[-1]
        ones = torch.ones(size, device=valid.device, dtype=torch.bool)
        return torch.cat([valid, ones], dim=-1)

    def _select(self, ratio: float, level: str):
        """-> (valid [L,1,Hkv,N] bool, thres float, r_real float); one host synchronisation."""
        self._flush_append()
        if "uniform" in level:
            self.valid, thres = self._threshold_uniform(self.score, ratio)
            n = self.valid.numel()
            k = int(self.valid.shape[-1] * ratio) if ratio < 1 else self.valid.shape[-1]
            kept = k * (n // self.valid.shape[-1])
        else:
            # scores still in the log buffer of the deferred scoring path: the launch that turns them into 16-bit values also
            # produces the first histogram of the selection (it streams every score anyway)
            hist = None
            buf = self._score_buf
            if (self._score is None and self._log_dirty and self._score_log is not None and buf is not None and buf.numel() > 0
                    and ratio < 1 and all(f == buf.shape[-1] for f in self._score_fill)):
                self._wait_score(finalize=False)
                hist = ops.select_workspace(buf.device)
                if not self._finalize_log(hist):
                    hist = None
            score = self._stacked_score(self.score)
            valid, thres_dev, kept_dev, _ = self._threshold_device(score, ratio, prehist=hist if score is buf else None)
            self.valid = valid.view(score.shape)
            host = torch.stack([thres_dev.double().squeeze(0), kept_dev.double().squeeze(0)]).cpu()  # one D2H sync
            if hist is not None and ratio < 1 and host[0] != host[0]:
                # a NaN threshold out of the pre-built histogram: either the rank lies inside the scores' NaNs (legitimate - every NaN
                # ranks above +inf, as in the reference's sort - and the plain path says the same) or the histogram was not of these scores (the kernels then flag the lost rank with NaN, kvz_select.hip)
                valid, thres_dev, kept_dev, _ = self._threshold_device(score, ratio)
                plain = torch.stack([thres_dev.double().squeeze(0), kept_dev.double().squeeze(0)]).cpu()
                if plain[0] == plain[0]:
                    raise ops.KvzError("selection: the histogram built by the finalize launch does not belong to these scores")
                self.valid, host = valid.view(score.shape), plain
            thres = float(host[0]) if ratio < 1 else 0.
            kept = int(host[1])
            n = self.valid.numel()
        assert self.valid.size(-1) == self.ctx_len
        # reference kvcache.py:133-134: rmv.float().mean() (fp32) -> 1 - python float
        r_ = 1 - float(np.float32(n - kept) / np.float32(n))
        self._evicted = n - kept
        return thres, r_


class EvictCache(_CacheBase):
    """KV cache that evicts KV from the cache before decoding (reference attention/kvcache.py:14-213)."""

    def __init__(self, model, evict_range: Tuple[int, int], device=None, dtype=None, layout: str = "slack",
                 slack: int = 1024, reserve: int = 4096, verbose: bool = True):
        super().__init__(model, evict_range, device=device, dtype=dtype, reserve=reserve)
        assert layout in ("slack", "packed")
        self.layout = layout
        self.slack = int(slack) if layout == "slack" else 0
        self.verbose = verbose
        self.info: Dict[str, Any] = {"flatten": False, "offset": None}
        self._attn_ws: Optional[torch.Tensor] = None
        self._dyn_off: Optional[torch.Tensor] = None   # device part of the appended-token count (graph-captured generation steps)
        self._dyn_val = 0                              # ... and what it holds, as the host knows it
        self._layout_epoch = 0                         # bumped whenever the flat cache moves (captured graphs hold its addresses)

    # reference: kvcache.py:41-80
    def update(self, key_states: torch.Tensor, value_states: torch.Tensor, layer_idx: int, cache_kwargs=dict()):
        """Update KV cache and return (K, V) of the layer."""
        if layer_idx == 0:
            seen_token = (cache_kwargs or {}).get("seen_token", key_states.size(-2))
            self._seen_tokens += seen_token

        if not self.info["flatten"]:
            self._dense_append(layer_idx, key_states, value_states)
        elif self.layout == "slack":
            t = key_states.size(-2)
            off = self.info["offset"][layer_idx]
            if off + t > self.slack:
                self._grow_slack(off + t)
            ops.append_inplace(self.key_cache[layer_idx], self.value_cache[layer_idx], key_states, value_states,
                               self.info["seg_start"][layer_idx], self.info["len_k"][layer_idx], off)
        else:  # packed: the reference's out-of-place rebuild (csrc/csrc/cuda_api.cu)
            cu_klen = self.info["cu_len_k"][layer_idx]
            head_lens = self.info["len_k"][layer_idx] + self.info["offset"][layer_idx]
            dim = key_states.size(-1)
            self.key_cache[layer_idx] = ops.update_flatten_view(
                self.key_cache[layer_idx], key_states.contiguous().view(-1, dim), head_lens, cu_klen)
            self.value_cache[layer_idx] = ops.update_flatten_view(
                self.value_cache[layer_idx], value_states.contiguous().view(-1, dim), head_lens, cu_klen)
        return self.key_cache[layer_idx], self.value_cache[layer_idx]

    # reference: kvcache.py:82-106
    def slice(self, seen_token_prev: int):
        """Evict KV of queries and generated tokens from the cache (for the reuse of the context cache)."""
        if not self.info["flatten"]:
            self._dense_slice(seen_token_prev)
        elif self.layout == "slack":
            pass  # appended rows live in the slack: resetting the offsets below is all it takes
        else:
            for l in range(self.n_layers):
                cu_klen = self.info["cu_len_k"][l].tolist()
                head_lens = self.info["len_k_host"][l]
                self.key_cache[l] = torch.cat(
                    [self.key_cache[l][cu_klen[h]:cu_klen[h] + head_lens[h]] for h in range(self.n_heads_kv)])
                self.value_cache[l] = torch.cat(
                    [self.value_cache[l][cu_klen[h]:cu_klen[h] + head_lens[h]] for h in range(self.n_heads_kv)])
                self.info["cu_len_k"][l] -= self.info["offset"][l] * self.info["cu_head"]
        self.info["offset"] = [0 for _ in range(self.n_layers)]
        self._seen_tokens = seen_token_prev

    # reference: kvcache.py:114-121
    def _mem(self) -> float:
        """Memory usage of the cache in GB (rows in use, K + V)."""
        mem = 0
        for l in range(len(self.key_cache)):
            if self.info["flatten"]:
                rows = self.info["rows_used"][l] + self.n_heads_kv * self.info["offset"][l]
                mem += rows * self.key_cache[l].shape[-1] * self.key_cache[l].element_size()
            else:
                mem += self.key_cache[l].numel() * self.key_cache[l].element_size()
        return round(2 * mem / 10**9, 1)

    # reference: kvcache.py:123-138
    def prune(self, ratio: float, level: str = "pair"):
        """Prune the KV cache.  -> (thres, real kept ratio).  On a cache that is pruned already: ``tighten``."""
        if self.pruned:
            return self.tighten(ratio, level)
        thres, r_ = self._select(ratio, level)
        self.prepare_init()
        self.pruned = True
        if self.verbose:
            print(f"ratio {r_:.2f} ({level}), {self._mem()} GB (evict {self._evicted:.0f} pairs)")
        return thres, r_

    # reference: kvcache.py:152-185
    def prepare_init(self):
        """Evict KV and prepare the varlen metadata: one plan + one gather launch for all layers."""
        self._flush_append()
        L, Hkv = self.n_layers, self.n_heads_kv
        klen = self.key_cache[0].shape[2]
        plan = ops.compact_plan(self.valid, self.sink, klen, slack=self.slack)
        meta = plan.meta.cpu()  # the single host sync of prepare_init
        o = 0
        len_h = meta[o:o + L * Hkv].view(L, Hkv); o += L * Hkv
        o += L * Hkv
        o += L * (Hkv + 1)
        max_h = meta[o:o + L]
        rows_used = len_h.sum(-1).tolist()
        totals = [r + Hkv * self.slack for r in rows_used]
        ks, vs = ops.compact_layers(self.key_cache, self.value_cache, plan, totals)
        self.key_cache, self.value_cache = list(ks), list(vs)
        self._store_k, self._store_v, self._fill = [], [], []  # release the dense storage
        self._views.clear()
        self._layout_epoch = getattr(self, "_layout_epoch", 0) + 1
        self._plan = plan
        cu_head = torch.arange(Hkv + 1, dtype=torch.int32, device=self.device)
        self.info = {
            "flatten": True,
            "layout": self.layout,
            "cu_head": cu_head,
            "len_k": [plan.len_k[l] for l in range(L)],          # kv lengths of heads in a layer (device int32)
            "len_k_host": len_h.tolist(),
            "max_len_k": [int(x) for x in max_h.tolist()],       # python ints: no per-step device sync
            "cu_len_k": [plan.cu_len_k[l].clone() for l in range(L)],  # packed-layout cumulative lengths
            "seg_start": [plan.seg_start[l] for l in range(L)],  # first row of each head segment
            "rows_used": rows_used,
            "offset": [0 for _ in range(L)],                     # rows appended after pruning, per layer
        }
        self._refresh_meta_host()

    def tighten(self, ratio: float, level: str = "pair"):
        """Prune an already pruned cache again, to a smaller ratio, from the rows it still holds (no reference counterpart: the
        reference prunes once).  -> (thres, real kept ratio), as ``prune``.  The scores stay on the device after the first prune and
        the masks of a falling ratio are nested at every level, so the new rows are gathered from the flat cache into fresh flat
        buffers (``kvz_recompact_layers``; peak memory old + new pruned cache) and the cache ends up as after ``prune(ratio, level)``
        on the dense K,V: same mask, lengths, segment starts and bytes.  Rows appended since the prune (``update_cache=True``) stay
        behind every head's rows (slack layout; the packed layout is re-laid out only while nothing is appended).  Two host
        synchronisations: the selection and the plan.  A ratio / level whose mask keeps a pair that was evicted raises ``ValueError``
        and leaves the cache as it was.  The flat cache moves: forks and captured decode graphs taken before raise as they do after
        a slack growth."""
        if not (self.pruned and self.info.get("flatten")):
            raise ops.KvzError("tighten: the cache is not pruned yet (prune() first)")
        L, Hkv = self.n_layers, self.n_heads_kv
        offsets = list(self.info["offset"])
        if self.layout == "packed" and any(offsets):
            raise ops.KvzError("tighten: the packed layout is re-laid out only while nothing is appended (slice() first, or use "
                               "layout='slack')")
        old_valid, old_evicted, old_plan = self.valid, self._evicted, self._plan
        try:
            thres, r_ = self._select(ratio, level)                       # host sync 1: threshold and kept count
            plan = ops.compact_plan(self.valid, self.sink, old_plan.klen, slack=self.slack)
            count = ops.mask_resurrects(self.valid, old_valid)
            meta = torch.cat([plan.meta, count]).cpu()                   # host sync 2: the plan and the subset check in one copy
            if int(meta[-1]):
                raise ValueError(f"tighten: ratio {ratio} ({level}) keeps {int(meta[-1])} KV pairs that were evicted before - a pruned "
                                 "cache can only be pruned further (same level, smaller ratio); prefill again for a larger one")
        except BaseException:
            self.valid, self._evicted = old_valid, old_evicted
            raise
        o = 0
        len_h = meta[o:o + L * Hkv].view(L, Hkv); o += 2 * L * Hkv + L * (Hkv + 1)
        max_h = meta[o:o + L]
        rows_used = len_h.sum(-1).tolist()
        totals = [r + Hkv * self.slack for r in rows_used]
        src = old_plan
        if self.slack != old_plan.slack:  # (the slack grew since the prune: the segments moved, the plan's other arrays hold)
            src = copy.copy(old_plan)
            src.seg_start, src.slack = torch.stack(self.info["seg_start"]), self.slack
        ks, vs = ops.recompact_layers(self.key_cache, self.value_cache, src, old_valid, plan, self.valid, totals, tail_rows=offsets)
        self.key_cache, self.value_cache = list(ks), list(vs)
        self._layout_epoch += 1
        self._plan = plan
        self.info = {
            "flatten": True,
            "layout": self.layout,
            "cu_head": self.info["cu_head"],
            "len_k": [plan.len_k[l] for l in range(L)],
            "len_k_host": len_h.tolist(),
            "max_len_k": [int(x) for x in max_h.tolist()],
            "cu_len_k": [plan.cu_len_k[l].clone() for l in range(L)],
            "seg_start": [plan.seg_start[l] for l in range(L)],
            "rows_used": rows_used,
            "offset": offsets,                                           # rows appended after pruning: carried over
        }
        self._refresh_meta_host()
        if self.verbose:
            print(f"ratio {r_:.2f} ({level}), {self._mem()} GB (evict {self._evicted:.0f} pairs)")
        return thres, r_

    def _refresh_meta_host(self):
        """ctypes copies [seg_start ++ len_k] per layer: passed by value to the attention kernel (slack layout only: in the packed
        layout the segment starts move with every appended token and live on the device)."""
        if self.layout != "slack":
            self.info["meta_host"] = None
            return
        seg = torch.stack(self.info["seg_start"]).cpu().tolist() if self.info["seg_start"] else []
        self.info["meta_host"] = [ops._meta_host(seg[l], self.info["len_k_host"][l], self.n_heads_kv) for l in range(self.n_layers)]

    def _grow_slack(self, need: int):
        """Re-lay out every layer with a larger slack (rare: only when more than ``slack`` tokens are appended)."""
        new_slack = max(2 * self.slack, need + 256)
        Hkv = self.n_heads_kv
        for l in range(self.n_layers):
            lens = self.info["len_k_host"][l]
            off = self.info["offset"][l]
            D = self.key_cache[l].shape[-1]
            total = sum(lens) + Hkv * new_slack
            nk = torch.empty((total, D), dtype=self.key_cache[l].dtype, device=self.device)
            nv = torch.empty((total, D), dtype=self.value_cache[l].dtype, device=self.device)
            old_start = self.info["seg_start"][l].tolist()
            starts, acc = [], 0
            for h in range(Hkv):
                starts.append(acc)
                n = lens[h] + off
                nk[acc:acc + n].copy_(self.key_cache[l][old_start[h]:old_start[h] + n])
                nv[acc:acc + n].copy_(self.value_cache[l][old_start[h]:old_start[h] + n])
                acc += lens[h] + new_slack
            self.key_cache[l], self.value_cache[l] = nk, nv
            self.info["seg_start"][l] = torch.tensor(starts, dtype=torch.int32, device=self.device)
        self.slack = new_slack
        self._layout_epoch += 1
        self._refresh_meta_host()

    # reference: kvcache.py:187-213
    def prepare(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor,
                layer_idx: int):
        """Flatten the queries for variable-length attention and bump the per-layer offsets."""
        bsz, n_heads_q, q_len, dim = query_states.shape
        cu_len_q = q_len * self.info["cu_head"]
        if q_len == 1:
            query_states = query_states.reshape(-1, self.n_group_kv, dim)  # pure view: [Hkv*1, G, D]
        else:
            query_states = query_states.view(bsz, self.n_heads_kv, self.n_group_kv, q_len, dim)
            query_states = query_states.transpose(2, 3).contiguous().view(-1, self.n_group_kv, dim)

        self.info["offset"][layer_idx] += q_len
        info = {
            "cu_len_q": cu_len_q,
            "max_len_q": q_len,
            "max_len_k": self.info["max_len_k"][layer_idx] + self.info["offset"][layer_idx],
            # MI355X layout: segment starts + base lengths + host-side offset
            "k_start": self.info["seg_start"][layer_idx],
            "k_len": self.info["len_k"][layer_idx],
            "k_len_offset": self.info["offset"][layer_idx],
            "meta_host": self._meta_host(layer_idx),
        }
        if self.layout == "packed":
            self.info["cu_len_k"][layer_idx] += cu_len_q
            info["cu_len_k"] = self.info["cu_len_k"][layer_idx]
            info["k_start"] = info["cu_len_k"][:-1]
        else:
            info["cu_len_k"] = None
        return query_states, key_states.view(-1, 1, dim), value_states.view(-1, 1, dim), info

    def attend(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor, info: dict,
               causal: bool = True, softmax_scale: Optional[float] = None) -> torch.Tensor:
        """Variable-length attention over the pruned cache: what the reference gets from
        ``flash_attn_varlen_func`` (attention/attn.py:61-71).  Returns ``[Hkv*q_len, G, D]``."""
        dim = query_states.shape[-1]
        ws = self._attn_workspace(info["max_len_q"], dim, query_states.device)
        return ops.varlen_attn(query_states, key_states.view(-1, dim), value_states.view(-1, dim), info["k_start"],
                               info["k_len"], info["max_len_q"], info["max_len_k"], causal=causal,
                               softmax_scale=softmax_scale, workspace=ws,
                               k_len_offset=info["k_len_offset"], meta_host=info.get("meta_host"))

    def _workspace(self, attr: str, key, make, args, need: int = 0, keep: Optional[int] = None) -> torch.Tensor:
        """Kernel scratch ``make(*args)`` from the lazily created dict ``attr`` of this cache: made at the first request for ``key``,
        and with a ``need`` again when the one at hand holds fewer elements or lives on another device than ``args[-1]``; a new key
        that finds more than ``keep`` others drops them all."""
        cache = getattr(self, attr, None)
        if cache is None:
            cache = {}
            setattr(self, attr, cache)
        ws = cache.get(key)
        if ws is None or (need and (ws.numel() < need or ws.device != torch.device(args[-1]))):
            if ws is None and keep is not None and len(cache) > keep:
                cache.clear()
            ws = cache[key] = make(*args)
        return ws

    def _attn_workspace(self, q_len: int, dim: int, device) -> torch.Tensor:
        """Zero-initialised scratch of the attention kernel, one per query length (its size does not depend on the key lengths)."""
        return self._workspace("_attn_ws_cache", (q_len, dim), ops.attn_workspace, (self.n_heads_kv, self.n_group_kv, q_len, dim, device),
                               keep=4)

    def _meta_host(self, layer_idx: int):
        """Head segments of a layer as kernel arguments (host copy made at prune / slack growth), or None."""
        mh = self.info.get("meta_host")
        return mh[layer_idx] if mh is not None else None

    def update_attend(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor, layer_idx: int,
                      softmax_scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Decode step (one new token) on the pruned cache, slack layout: ``update`` + ``prepare`` + ``attend`` in one
        launch of the attention kernel, which also writes the token's K, V row into the slack of every head.
        query ``[1, H, 1, D]``, key / value ``[1, Hkv, 1, D]``; returns ``[Hkv, G, D]`` like ``attend``.  The cache
        bookkeeping (``_seen_tokens``, ``info["offset"]``) ends up exactly as after the three separate calls."""
        assert self.info["flatten"] and self.layout == "slack" and query_states.shape[-2] == 1
        if layer_idx == 0:
            self._seen_tokens += 1
        off = self.info["offset"][layer_idx]
        if off + 1 > self.slack:
            self._grow_slack(off + 1)
        dim = query_states.shape[-1]
        max_len_k = self.info["max_len_k"][layer_idx] + off + 1
        ws = self._attn_workspace(1, dim, query_states.device)
        # (the appended-token count = host part + device part: see decode_graph; without a graph there is no device part)
        if self._dyn_off is not None and off < self._dyn_val:  # (after slice(): the device part restarts with the host's count)
            self._sync_dyn(off)
        out = ops.varlen_attn_append(query_states.reshape(-1, self.n_group_kv, dim), self.key_cache[layer_idx],
                                     self.value_cache[layer_idx], key_states, value_states,
                                     self.info["seg_start"][layer_idx], self.info["len_k"][layer_idx], off - self._dyn_val, max_len_k,
                                     softmax_scale=softmax_scale, workspace=ws, meta_host=self._meta_host(layer_idx),
                                     offset_dev=self._dyn_off, out=out)
        self.info["offset"][layer_idx] = off + 1
        return out

    # ---- speculative decoding: verify t drafted positions in one step, take the rejected ones back ------------------------------
    @contextlib.contextmanager
    def verifying(self, tree=None):
        """While inside, a forward pass of 2 .. 64 // G tokens on this pruned slack-layout cache takes ``verify_attend``
        (kvzip_amd.attn).  Only the speculative loop sets it: without it every forward goes where it always went.  ``tree=parents``
        (``parents[0] = -1``, ``parents[i] < i``): the ``len(parents)`` tokens of such a forward are the nodes of a tree, node i
        continuing node ``parents[i]``, and ``verify_attend`` masks the new rows by ancestry (``kvz_tree_attn_append``);
        ``keep_path`` afterwards keeps the rows of the accepted path."""
        # (raises for what is no tree before anything is set; converted once for the calls of all layers)
        anc = ops.mask_array(ops.ancestor_masks(tree)) if tree is not None else None
        prev, self._verifying = getattr(self, "_verifying", False), True
        prev_anc, self._verify_anc = getattr(self, "_verify_anc", None), anc
        try:
            yield self
        finally:
            self._verifying, self._verify_anc = prev, prev_anc

    def verify_attend(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor, layer_idx: int,
                      softmax_scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Verify step (t consecutive new positions) on the pruned cache, slack layout: ``update`` + ``prepare`` + ``attend`` for
        ``q_len = t`` in one call of ``kvz_spec_attn_append``, which reads the kept rows once (twice beyond 32 query rows per KV
        head) and writes the t K,V rows into the slack of every head.  query ``[1, H, t, D]``, key / value ``[1, Hkv, t, D]``;
        returns ``[Hkv*t, G, D]`` like ``attend``.  The cache bookkeeping (``_seen_tokens``, ``info["offset"]``) ends up exactly as
        after the three separate calls; ``rewind`` takes positions back.  Inside ``verifying(tree=parents)`` the t positions are the
        nodes of that tree and the call is ``kvz_tree_attn_append``: same rows written, node p attends to its ancestors among them."""
        assert self.info["flatten"] and self.layout == "slack" and query_states.shape[0] == 1
        t, dim = query_states.shape[-2], query_states.shape[-1]
        Hkv, G = self.n_heads_kv, self.n_group_kv
        anc = getattr(self, "_verify_anc", None)
        if anc is not None and len(anc) != t:
            raise ops.KvzError(f"verify_attend: a forward pass of {t} tokens inside verifying(tree=...) of {len(anc)} nodes")
        if layer_idx == 0:
            self._seen_tokens += t
        off = self.info["offset"][layer_idx]
        if off + t > self.slack:
            self._grow_slack(off + t)
        q = query_states.reshape(Hkv, G, t, dim).transpose(1, 2).contiguous()                   # [Hkv, t, G, D]: row = p*G + g
        ws = self._spec_workspace(t, dim, query_states.device)
        if out is not None:
            out = out.view(Hkv, t, G, dim)
        if anc is not None:
            out = ops.tree_attn_append(q, self.key_cache[layer_idx], self.value_cache[layer_idx], self.info["seg_start"][layer_idx],
                                       self.info["len_k"][layer_idx], off, self.slack, key_states[0], value_states[0], anc,
                                       softmax_scale=softmax_scale, workspace=ws, meta_host=self._meta_host(layer_idx), out=out)
        else:
            out = ops.spec_attn_append(q, self.key_cache[layer_idx], self.value_cache[layer_idx], self.info["seg_start"][layer_idx],
                                       self.info["len_k"][layer_idx], off, self.slack, key_states[0], value_states[0],
                                       softmax_scale=softmax_scale, workspace=ws, meta_host=self._meta_host(layer_idx), out=out)
        self.info["offset"][layer_idx] = off + t
        return out.view(Hkv * t, G, dim)

    def _spec_workspace(self, t: int, dim: int, device) -> torch.Tensor:
        """Scratch of the verify step, one per number of 16-row tiles (its size depends on nothing else that changes between steps)."""
        need = int(ops._lib.load().kvz_spec_attn_workspace_bytes(t, self.n_heads_kv, self.n_group_kv, dim))
        return self._workspace("_spec_ws_cache", ((t * self.n_group_kv + 15) // 16, dim), ops.spec_attn_workspace,
                               (t, self.n_heads_kv, self.n_group_kv, dim, device), need=need)

    def rewind(self, n: int) -> None:
        """Take back the last ``n`` appended positions (the rejected tail of a verify step): a host-side decrement of every layer's
        offset and of ``_seen_tokens``, no launch.  The rows stay in the slack as garbage, exactly as after ``slice``, and the next
        appended token overwrites them.  Slack layout only; ``n`` may not exceed what was appended since the prune or the last
        ``slice``."""
        n = int(n)
        if not (self.info.get("flatten") and self.layout == "slack"):
            raise ops.KvzError("rewind: only a pruned slack-layout cache takes appended positions back on the host (a dense or "
                               "packed-layout cache: slice())")
        have = min(self.info["offset"])
        if n < 0 or n > have:
            raise ops.KvzError(f"rewind: {n} positions, but {have} were appended since the prune or the last slice")
        self.info["offset"] = [o - n for o in self.info["offset"]]
        self._seen_tokens -= n

    def keep_path(self, path, t: int) -> None:
        """After a tree verify step of ``t`` nodes (``verifying(tree=...)``): keep the rows of the accepted path - ``path`` ascending
        node indices, ``path[i] >= i`` - in the first ``len(path)`` of the t slots behind every head segment, in every layer (one
        ``kvz_tree_keep_path`` launch for all layers, none for an identity path), and take the other ``t - len(path)`` positions back
        (``rewind``).  Called between forward passes.  ``KvzError`` before anything is touched for a cache that is not a pruned
        slack-layout one, offsets that differ between layers or are below ``t``, or a bad path."""
        t = int(t)
        path = [int(x) for x in path]
        if not (self.info.get("flatten") and self.layout == "slack"):
            raise ops.KvzError("keep_path: only a pruned slack-layout cache holds the node rows of a tree verify step behind its segments")
        offs = self.info["offset"]
        if min(offs) != max(offs):
            raise ops.KvzError(f"keep_path: the layers hold different numbers of appended positions ({min(offs)} .. {max(offs)}): call it "
                               "between forward passes")
        if not 1 <= t <= ops.TREE_MAX_NODES or offs[0] < t:
            raise ops.KvzError(f"keep_path: t = {t} node rows, but {offs[0]} positions were appended since the prune or the last slice "
                               f"(1 .. {ops.TREE_MAX_NODES} nodes)")
        for i, x in enumerate(path):
            if x < i or x >= t or (i and x <= path[i - 1]):
                raise ops.KvzError(f"keep_path: path[{i}] = {x}: a path is strictly ascending with i <= path[i] < t = {t}")
        if any(x != i for i, x in enumerate(path)):
            Hkv, base = self.n_heads_kv, offs[0] - t
            row0 = []
            for l in range(self.n_layers):
                mh = self._meta_host(l)
                starts = list(mh[:Hkv]) if mh is not None else self.info["seg_start"][l].tolist()
                row0 += [starts[h] + self.info["len_k_host"][l][h] + base for h in range(Hkv)]
            ops.tree_keep_path(self.key_cache, self.value_cache, row0, path, t)
        self.rewind(t - len(path))

    def fork(self, n_branches: int, tail_capacity: int = 256) -> "ForkedCache":
        """``n_branches`` concurrent queries over this pruned cache: the branches share its rows read-only and each owns a private
        tail for the K,V of its query and of its answer (see ``ForkedCache``)."""
        return ForkedCache(self, n_branches, tail_capacity=tail_capacity)

    # ---- a whole generation step as ONE HIP graph ---------------------------------------------------------------------------
    def decode_graph(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, softmax_scale: Optional[float] = None):
        """Capture the attention part of ONE generation step over all layers - L x (append the token's K,V + variable-length
        attention) - into a HIP graph and return a ``DecodeGraph``; ``replay()`` runs the step for the tensors that are in the
        static buffers at that moment (``query [L, 1, H, 1, D]``, ``key`` / ``value [L, 1, Hkv, 1, D]``; outputs in ``.out``
        ``[L, Hkv, G, D]``).  Replays need unchanged kernel arguments, so the part of the appended-token count that changes from
        token to token lives in a device counter that the last node of the graph advances (``k_len_offset_dev``); the host
        bookkeeping (``info["offset"]``, ``_seen_tokens``) advances in ``replay()``.  What a serving engine does with its
        static input buffers; the per-layer hooks of a Python forward pass (``update_attend``) stay available beside it."""
        assert self.info["flatten"] and self.layout == "slack"
        L = self.n_layers
        assert query.shape[0] == L and key.shape[0] == L and value.shape[0] == L and query.shape[-2] == 1
        lib = ops._lib.load()
        offsets0, seen0 = list(self.info["offset"]), self._seen_tokens
        assert min(offsets0) == max(offsets0), "a generation step starts with the same number of appended tokens in every layer"
        if offsets0[0] + 2 > self.slack:
            self._grow_slack(offsets0[0] + 2)
        if self._dyn_off is None:
            self._dyn_off = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._sync_dyn(offsets0[0])   # the WHOLE count lives on the device from here on: the captured host part is 0
        out = torch.empty((L, self.n_heads_kv, self.n_group_kv, query.shape[-1]), dtype=query.dtype, device=query.device)
        ws = self._attn_workspace(1, query.shape[-1], query.device)
        dyn0 = self._dyn_val
        torch.cuda.synchronize(query.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for l in range(L):
                self.update_attend(query[l], key[l], value[l], l, softmax_scale=softmax_scale, out=out[l])
            ops.check(lib.kvz_add_i32(self._dyn_off.data_ptr(), 1, ops._stream(self._dyn_off)), "kvz_add_i32")
        # (capturing executes nothing: the host bookkeeping goes back to where it was)
        self.info["offset"], self._seen_tokens, self._dyn_val = offsets0, seen0, dyn0
        # the captured kernels hold RAW ADDRESSES: the graph object keeps every tensor behind them alive (the shared attention
        # workspace may be dropped from the cache's own table by later calls with other query lengths, the static input buffers
        # belong to the caller)
        pinned = (ws, self._dyn_off, query, key, value, list(self.key_cache), list(self.value_cache),
                  list(self.info["seg_start"]), list(self.info["len_k"]))
        return DecodeGraph(self, graph, out, pinned)

    def _sync_dyn(self, value: int):
        """device part of the appended-token count := value (one fill on the current stream)"""
        if self._dyn_val != value or value == 0:
            self._dyn_off.fill_(value)
            self._dyn_val = value


class DecodeGraph:
    """One captured generation step of an ``EvictCache`` (see ``EvictCache.decode_graph``)."""

    def __init__(self, kv: "EvictCache", graph, out: torch.Tensor, pinned=()):
        self.kv, self.graph, self.out = kv, graph, out
        self.epoch = kv._layout_epoch
        self._pinned = pinned   # every tensor whose address a captured kernel holds (see decode_graph)

    def replay(self) -> torch.Tensor:
        kv = self.kv
        off = kv.info["offset"]
        if self.epoch != kv._layout_epoch:
            raise ops.KvzError("decode graph: the flat cache was re-laid out since the capture (prune / slack growth): capture again")
        if max(off) + 1 > kv.slack:
            raise ops.KvzError("decode graph: the slack of the head segments is used up (the graph holds the addresses of the flat "
                               "cache: grow the slack and capture again)")
        assert min(off) == max(off)
        if off[0] != kv._dyn_val:  # (tokens appended by the per-layer hooks, or slice(), since the last replay)
            kv._sync_dyn(off[0])
        self.graph.replay()
        kv.info["offset"] = [o + 1 for o in off]
        kv._seen_tokens += 1
        kv._dyn_val += 1
        return self.out


def plan_branch_reorder(parents: Sequence[int], n_slots: int) -> Tuple[List[int], List[Tuple[int, int]]]:
    """Where the hypotheses of a beam-search step live and what has to be copied for it (pure host logic, deterministic).
    ``parents[i]`` is the branch slot whose state hypothesis i continues (at most ``n_slots`` hypotheses; a parent may appear several
    times or not at all).  -> ``(slots, pairs)``: hypothesis i lives in ``slots[i]`` afterwards and ``pairs`` lists the
    ``(src, dst)`` slot copies that make it so.  The first child of a parent stays in the parent's slot, with no copy; every further
    child goes to a slot whose occupant has no child, lowest slot first.  A pure permutation of survivors therefore costs nothing, the
    number of copies is the number of children beyond each parent's first (with all slots in use: the number of dropped hypotheses),
    and sources (slots with a child) and destinations (slots without) are disjoint by construction - what the in-place copy of
    ``kvz_fork_branch_copy`` needs."""
    parents = [int(p) for p in parents]
    n_slots = int(n_slots)
    if len(parents) > n_slots:
        raise ValueError(f"plan_branch_reorder: {len(parents)} hypotheses for {n_slots} slots")
    for p in parents:
        if not 0 <= p < n_slots:
            raise ValueError(f"plan_branch_reorder: parent slot {p} outside [0, {n_slots})")
    has_child = set(parents)
    free = [s for s in range(n_slots) if s not in has_child]      # ascending: lowest slot first
    slots: List[int] = []
    pairs: List[Tuple[int, int]] = []
    kept = set()
    for p in parents:
        if p not in kept:
            kept.add(p)
            slots.append(p)
        else:
            d = free.pop(0)                                        # (there is one: every hypothesis beyond a parent's first leaves a slot childless)
            slots.append(d)
            pairs.append((p, d))
    return slots, pairs


def pruned_slack(c):
    """Whether (truthy or falsy) the ``EvictCache`` ``c`` is pruned into the flat slack layout: what a fork shares, a batch appends to and a verify
    step rewinds."""
    return c.pruned and c.info.get("flatten") and c.layout == "slack"


def _decode_rows(key_states: torch.Tensor, value_states: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The new K and V rows ``[B, Hkv, 1, D]`` of a batched decode step as its kernels read them: unit stride along D, batch and head
    strides multiples of 8 elements.  Copied only when the strides require it."""
    (kb, kh, _, kd), (vb, vh, _, vd) = key_states.stride(), value_states.stride()
    if kd != 1 or vd != 1 or kb % 8 or kh % 8 or vb % 8 or vh % 8:
        return key_states.contiguous(), value_states.contiguous()
    return key_states, value_states


class _Slots:
    """The slot protocol ``ForkedCache`` (a slot is a branch) and ``CacheBatch`` (a slot is a member) share: ``active`` says which
    slots are live (its length is the slot count), ``retire`` ends one, and ``select_packed`` names the slots whose query tokens the
    next forward pass carries back to back (``_packed``; cleared after the last layer's call).  ``_nouns`` words the messages."""

    _nouns: Tuple[str, str, str, str, str]   # who raises, its short name, a slot, several slots, where a slot's rows land
    active: List[bool]
    _packed: Optional[Tuple[List[int], List[int]]] = None   # (slots, lengths) of the next forward pass

    def select_packed(self, slots: Sequence[int], lengths: Sequence[int]) -> None:
        """The next forward pass carries the queries of ``slots`` (distinct, live) back to back, ``lengths[i]`` tokens of ``slots[i]``
        each: every layer's ``first_step`` then takes ``sum(lengths)`` positions.  Cleared after the last layer's call."""
        who, short, one, many, home = self._nouns
        slots, lengths = [int(b) for b in slots], [int(n) for n in lengths]
        if len(slots) != len(lengths):
            raise ops.KvzError(f"{who}: select_packed got {len(slots)} {many} and {len(lengths)} lengths")
        if not slots:
            raise ops.KvzError(f"{who}: select_packed needs at least one {one}")
        if len(set(slots)) != len(slots):
            raise ops.KvzError(f"{who}: select_packed names a {one} twice ({slots}): its rows would land in one {home} twice")
        for b, n in zip(slots, lengths):
            if not 0 <= b < len(self.active):
                raise ops.KvzError(f"{who}: select_packed: no {one} {b} (the {short} has {len(self.active)})")
            if not self.active[b]:
                raise ops.KvzError(f"{who}: select_packed: {one} {b} is retired")
            if n < 0:
                raise ops.KvzError(f"{who}: select_packed: {one} {b} has a negative length {n}")
        self._packed = (slots, lengths)

    def retire(self, b: int) -> None:
        """Slot ``b`` is finished (EOS, token budget): later decode steps skip it (no write, zero output rows)."""
        self.active[b] = False

    def _packing(self, query_states: torch.Tensor):
        """The selected packing for ``[1, H, T, D]`` queries -> ``(slots, lengths, order, cu)``: ``order`` lists the slots in packing
        order, then those that take no part; ``cu[i] .. cu[i + 1]`` are the positions of ``order[i]`` (empty runs at the end)."""
        slots, lengths = self._packed
        bsz, T = query_states.shape[0], query_states.shape[2]
        if bsz != 1 or T != sum(lengths):
            raise ops.KvzError(f"{self._nouns[0]}: the packed first step takes [1, H, {sum(lengths)}, D] queries, the lengths "
                               f"{lengths} of {self._nouns[3]} {slots} back to back (got batch {bsz}, {T} positions)")
        order = slots + [b for b in range(len(self.active)) if b not in slots]
        cu = [0]
        for n in lengths:
            cu.append(cu[-1] + n)
        cu += [T] * (len(self.active) - len(slots))
        return slots, lengths, order, cu

    def _packing_done(self, layer_idx: int) -> None:
        if layer_idx == self.n_layers - 1:
            self._packed = None


class ForkedCache(_Slots):
    """``n_branches`` concurrent queries over ONE pruned slack-layout ``EvictCache`` (``EvictCache.fork``; no reference counterpart:
    batch is 1 there).  The branches share the base cache's flat K,V read-only - its rows, segment starts and lengths as they were at
    the fork, rows a multi-turn ``update_cache=True`` appended before it included - and every branch owns a private tail per layer
    (``[B, Hkv, tail_capacity, D]``: the K,V of its query tokens and of the tokens it generates).  One decode step of all live
    branches is one attention launch per layer that reads the shared rows once (``kvz_fork_attn_append``).

    Hooks for the attention adapter (``kvzip_amd.attn``):
      * ``first_step`` - the query of ONE branch (``select_branch`` names it), ``q_len > 1``: ``kvz_flash_fwd`` over the shared
        segments (no mask) and over the branch's tail (causal), merged by their LSEs; or, after ``select_packed``, the queries of
        SEVERAL branches back to back in one pass: one ``kvz_flash_fwd`` over the shared segments for all positions and one
        ``kvz_fork_prefill_tail`` for everything branch-private (append, causal attention inside each branch's tail, merge);
      * ``update_attend`` - ``[B, H, 1, D]`` queries, one new token per live branch.
    The fork never changes ``info["offset"]``, ``_seen_tokens`` or any row of the base cache - until ``commit`` moves ONE branch's
    rows into the base's slack and closes the fork.  A prune or a slack growth of the base moves the rows the fork points at: every
    hook then raises ``KvzError`` (as ``DecodeGraph.replay`` does).

    Beam search: ``reorder(parents)`` makes "hypothesis i continues from slot ``parents[i]``" true between two decode steps by copying
    whole tails between slots (``kvz_fork_branch_copy``: survivors stay where they are, one copy per dropped hypothesis)."""

    _nouns = ("forked cache", "fork", "branch", "branches", "tail")
    _closed = False   # commit() sets it on the instance: one branch's rows now belong to the base and every later hook raises

    @staticmethod
    def check_base(base, n_branches: int) -> None:
        """Raise ``KvzError`` unless ``base`` can be forked into ``n_branches`` (what ``__init__`` asks; a caller that appends rows to
        the base before it forks asks first, so that a refusal leaves the base as it was)."""
        if not (isinstance(base, EvictCache) and pruned_slack(base)):
            raise ops.KvzError("fork: needs a pruned EvictCache in the slack layout")
        G = base.n_group_kv
        if n_branches < 1 or n_branches > ops.FORK_MAX_BRANCHES or n_branches * G > ops.FORK_MAX_ROWS:
            raise ops.KvzError(f"fork: {n_branches} branches x {G} query heads per KV head: one launch takes at most "
                               f"{ops.FORK_MAX_ROWS} query rows per KV head and {ops.FORK_MAX_BRANCHES} branches")
        if base.n_heads_kv > 64:
            raise ops.KvzError("fork: more than 64 KV heads")

    def __init__(self, base: "EvictCache", n_branches: int, tail_capacity: int = 256):
        self.check_base(base, n_branches)
        G = base.n_group_kv
        offs = base.info["offset"]
        self.base, self.n_branches = base, int(n_branches)
        self.n_layers, self.n_heads_kv, self.n_group_kv = base.n_layers, base.n_heads_kv, G
        self.device, self.dtype = base.device, base.dtype
        self.pruned, self.get_score, self.layout = True, False, "fork"
        self._epoch = base._layout_epoch
        self._offset = list(offs)                                   # rows appended to the base before the fork, per layer
        self._k = list(base.key_cache)                              # references: the storage outlives a re-layout of the base
        self._v = list(base.value_cache)
        self._seg = list(base.info["seg_start"])
        self._len = list(base.info["len_k"])
        self._meta = list(base.info["meta_host"])
        seg = [list(m[:self.n_heads_kv]) for m in self._meta]
        self._starts = seg
        self._lens = [[n + self._offset[l] for n in base.info["len_k_host"][l]] for l in range(self.n_layers)]
        self.tail_capacity = max(int(tail_capacity), 1)
        self.tail_k: List[Optional[torch.Tensor]] = [None] * self.n_layers   # allocated at a layer's first use (the head dim is the call's)
        self.tail_v: List[Optional[torch.Tensor]] = [None] * self.n_layers
        self.tail_len = [[0] * self.n_branches for _ in range(self.n_layers)]
        self.active = [True] * self.n_branches
        self._branch = 0
        self._packed = None
        self._ws = None

    # -- bookkeeping ---------------------------------------------------------------------------------
    def get_seq_length(self, layer_idx: Optional[int] = 0) -> int:
        return self.base.get_seq_length(layer_idx)

    def select_branch(self, b: int) -> None:
        """The branch the next ``first_step`` calls belong to."""
        assert 0 <= b < self.n_branches
        self._branch = int(b)

    def _check(self, layer_idx: int) -> None:
        base = self.base
        if self._closed:
            raise ops.KvzError("forked cache: the fork is closed (commit() moved a branch into the base cache): fork again")
        if self._epoch != base._layout_epoch or not base.info.get("flatten"):
            raise ops.KvzError("forked cache: the base cache was re-laid out since the fork (prune / slack growth): fork again")
        if base.info["offset"][layer_idx] < self._offset[layer_idx]:
            raise ops.KvzError("forked cache: the base cache was sliced below the rows it held at the fork: fork again")

    def _tails(self, layer_idx: int, need: int, D: int):
        """The layer's tails with room for ``need`` rows per branch (re-allocated with at least twice the capacity when outgrown)."""
        tk = self.tail_k[layer_idx]
        if tk is None or tk.shape[2] < need:
            cap = self.tail_capacity if tk is None else tk.shape[2]
            while cap < need:
                cap *= 2
            shape = (self.n_branches, self.n_heads_kv, cap, D)
            nk = torch.empty(shape, dtype=self.dtype, device=self.device)
            nv = torch.empty(shape, dtype=self.dtype, device=self.device)
            if tk is not None:
                nk[:, :, :tk.shape[2]].copy_(tk)
                nv[:, :, :tk.shape[2]].copy_(self.tail_v[layer_idx])
            self.tail_k[layer_idx], self.tail_v[layer_idx] = nk, nv
            self.tail_capacity = max(self.tail_capacity, cap)
        return self.tail_k[layer_idx], self.tail_v[layer_idx]

    # -- beam search / keeping a branch ---------------------------------------------------------------------
    def reorder(self, parents: Sequence[int]) -> List[int]:
        """Continue hypothesis i from the state of branch slot ``parents[i]`` (a live slot; it may be named several times or not at
        all): plan (``plan_branch_reorder``) and copy (``kvz_fork_branch_copy``: one launch for all layers) in one call.  -> ``slots``,
        the slot hypothesis i lives in afterwards; the caller permutes its per-slot state (tokens, scores, positions) by it.  A
        destination takes its source's tail rows and tail length in every layer and is live; slots left without a hypothesis are
        retired.  Called between forward passes: a source's tail length must be the same in every layer."""
        if self._packed is not None:
            raise ops.KvzError("forked cache: reorder while a packing is selected (the packed first step has not run in every layer)")
        for l in range(self.n_layers):
            self._check(l)
        parents = [int(p) for p in parents]
        if len(parents) > self.n_branches:
            raise ops.KvzError(f"forked cache: reorder got {len(parents)} hypotheses, the fork has {self.n_branches} slots")
        for p in parents:
            if not 0 <= p < self.n_branches:
                raise ops.KvzError(f"forked cache: reorder: no branch {p} (the fork has {self.n_branches})")
            if not self.active[p]:
                raise ops.KvzError(f"forked cache: reorder: branch {p} is retired, nothing continues from it")
        slots, pairs = plan_branch_reorder(parents, self.n_branches)
        rows = []
        for s, _ in pairs:
            n = self.tail_len[0][s]
            if any(self.tail_len[l][s] != n for l in range(self.n_layers)):
                raise ops.KvzError(f"forked cache: reorder in the middle of a forward pass (the tail of branch {s} holds "
                                   f"{[self.tail_len[l][s] for l in range(self.n_layers)]} rows per layer)")
            rows.append(n)
        if pairs and max(rows) > 0:
            if any(t is None for t in self.tail_k):
                raise ops.KvzError("forked cache: reorder: a layer's tails hold rows but were never allocated")
            ops.fork_branch_copy(self.tail_k, self.tail_v, pairs, rows)
        for (s, d), n in zip(pairs, rows):
            for l in range(self.n_layers):
                self.tail_len[l][d] = n
        live = set(slots)
        self.active = [b in live for b in range(self.n_branches)]
        return slots

    def commit(self, b: int) -> None:
        """Keep branch ``b``: append its tail rows, all layers, to the BASE cache behind every head's current rows
        (``kvz_append_inplace``, one call per layer, reading the tail through its own strides - no intermediate copy), growing the
        base's slack first where needed.  Afterwards the base is exactly as after its own ``update`` of that many tokens
        (``info["offset"]`` and ``_seen_tokens`` advanced by the branch's tail length) and the fork is closed: every later hook raises
        ``KvzError``.  Nothing else of the base changes."""
        if self._packed is not None:
            raise ops.KvzError("forked cache: commit while a packing is selected")
        b = int(b)
        if not 0 <= b < self.n_branches:
            raise ops.KvzError(f"forked cache: commit: no branch {b} (the fork has {self.n_branches})")
        base = self.base
        for l in range(self.n_layers):
            self._check(l)
            if base.info["offset"][l] != self._offset[l]:
                raise ops.KvzError("forked cache: commit: rows were appended to the base cache since the fork (its slack behind the "
                                   "rows the fork shares is not free): slice it back first")
        t = self.tail_len[0][b]
        if any(self.tail_len[l][b] != t for l in range(self.n_layers)):
            raise ops.KvzError(f"forked cache: commit in the middle of a forward pass (the tail of branch {b} holds "
                               f"{[self.tail_len[l][b] for l in range(self.n_layers)]} rows per layer)")
        if t > 0:
            if max(self._offset) + t > base.slack:
                base._grow_slack(max(self._offset) + t)        # (the flat cache moves: this fork is closed below anyway)
            for l in range(self.n_layers):
                ops.append_inplace(base.key_cache[l], base.value_cache[l], self.tail_k[l][b:b + 1, :, :t], self.tail_v[l][b:b + 1, :, :t],
                                   base.info["seg_start"][l], base.info["len_k"][l], self._offset[l])
                base.info["offset"][l] = self._offset[l] + t
            base._seen_tokens += t
        self._closed = True

    # -- hooks ------------------------------------------------------------------------------------------
    def first_step(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor, layer_idx: int,
                   softmax_scale: Optional[float] = None) -> torch.Tensor:
        """The query of the selected branch: query ``[1, H, q, D]``, key / value ``[1, Hkv, q, D]``.  Appends the K,V rows to the
        branch's tail and returns the attention over shared segment ++ tail (bottom-right causal inside the tail) as
        ``[Hkv, q, G, D]``.  With a packing selected (``select_packed``): the queries of its branches back to back, same shapes with
        ``q = sum(lengths)``; every branch's rows go to its own tail and see only the shared segments and that tail."""
        self._check(layer_idx)
        if self._packed is not None:
            return self._first_step_packed(query_states, key_states, value_states, layer_idx, softmax_scale)
        b = self._branch
        bsz, _, q_len, D = query_states.shape
        if bsz != 1:
            raise ops.KvzError("forked cache: the first step of a branch runs at batch 1")
        Hkv = self.n_heads_kv
        t = self.tail_len[layer_idx][b]
        tk, tv = self._tails(layer_idx, t + q_len, D)
        cap = tk.shape[2]
        if key_states.stride(-1) != 1 or value_states.stride(-1) != 1:
            key_states, value_states = key_states.contiguous(), value_states.contiguous()
        lib = ops._lib.load()
        rc = lib.kvz_dense_append(tk[b].data_ptr(), tv[b].data_ptr(), cap * D, t, key_states.data_ptr(), value_states.data_ptr(),
                                  key_states.stride(1), key_states.stride(2), value_states.stride(1), value_states.stride(2),
                                  Hkv, q_len, D, tk.element_size(), ops._stream(tk))
        ops.check(rc, "kvz_dense_append")
        o1, l1 = ops.flash_fwd_ragged(query_states, self._k[layer_idx], self._v[layer_idx], self._starts[layer_idx],
                                      self._lens[layer_idx], causal=False, softmax_scale=softmax_scale)
        o2, l2 = ops.flash_fwd_ragged(query_states, tk[b].view(-1, D), tv[b].view(-1, D), [h * cap for h in range(Hkv)],
                                      [t + q_len] * Hkv, causal=True, softmax_scale=softmax_scale)
        self.tail_len[layer_idx][b] = t + q_len
        return ops.attn_merge_lse(o1, l1, o2, l2, out=o1)

    def _first_step_packed(self, query_states, key_states, value_states, layer_idx, softmax_scale):
        branches, lengths, order, cu = self._packing(query_states)
        D = query_states.shape[-1]
        tlen = self.tail_len[layer_idx]
        tk, tv = self._tails(layer_idx, max(tlen[b] + n for b, n in zip(branches, lengths)), D)
        o, lse = ops.flash_fwd_ragged(query_states, self._k[layer_idx], self._v[layer_idx], self._starts[layer_idx],
                                      self._lens[layer_idx], causal=False, softmax_scale=softmax_scale)
        ops.fork_prefill_tail(query_states, cu, tk, tv, tlen, key_states, value_states, o, lse, softmax_scale=softmax_scale, out=o,
                              branches=order)
        for b, n in zip(branches, lengths):
            tlen[b] += n
        self._packing_done(layer_idx)
        return o

    def update_attend(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor, layer_idx: int,
                      softmax_scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Decode step of all branches: query ``[B, H, 1, D]``, key / value ``[B, Hkv, 1, D]`` -> ``[B, Hkv, G, D]``.  Live branches
        get their new row appended to their tail; retired ones are skipped (their output rows are zero)."""
        self._check(layer_idx)
        B, _, q_len, D = query_states.shape
        if B != self.n_branches or q_len != 1:
            raise ops.KvzError(f"forked cache: a decode step takes [{self.n_branches}, H, 1, D] queries (got batch {B}, {q_len} positions)")
        lens = self.tail_len[layer_idx]
        tk, tv = self._tails(layer_idx, max(lens) + 1, D)
        key_states, value_states = _decode_rows(key_states, value_states)
        if self._ws is None or self._ws[0] != D:
            self._ws = (D, ops.fork_attn_workspace(B, self.n_heads_kv, self.n_group_kv, D, self.device))
        q = query_states.reshape(B, self.n_heads_kv, self.n_group_kv, D).contiguous()
        tl = [n if a else -1 for n, a in zip(lens, self.active)]
        out = ops.fork_attn_append(q, self._k[layer_idx], self._v[layer_idx], self._seg[layer_idx], self._len[layer_idx],
                                   self._offset[layer_idx], tk, tv, tl, key_states, value_states, softmax_scale=softmax_scale,
                                   workspace=self._ws[1], meta_host=self._meta[layer_idx], out=out)
        for b in range(B):
            if self.active[b]:
                lens[b] += 1
        return out


class CacheBatch(_Slots):
    """Several INDEPENDENT pruned slack-layout ``EvictCache`` objects decoding together, one token each per step (no reference
    counterpart: batch is 1 there).  Several users, each with an own compressed context: one decode step of all live members is one
    attention launch per layer (``kvz_multi_attn_append``), whose work items are cut from the sum of ALL members' head lengths.

    The batch owns no rows and no state of its members: every member keeps its own rows in its own slack, and after a step every
    live member is exactly as after its own ``EvictCache.update_attend`` - the new row in its slack, ``info["offset"][layer]``
    advanced by one, ``_seen_tokens`` advanced at layer 0.  A member can therefore be used alone, sliced, tightened or continued with
    ``update_cache=True`` between or after the steps.  A member whose layout changed since the last step (slack growth, ``tighten``)
    makes the batch rebuild its segment table (host arrays of addresses, starts and lengths; no tensor of a member is held between
    calls).  Offsets may differ between members and between calls.

    Hooks for the attention adapter (``kvzip_amd.attn``):
      * ``update_attend`` - ``[B, H, 1, D]`` queries, one new token per live member;
      * ``first_step`` - after ``select_packed``: the query tokens of several members back to back in ONE batch-1 pass
        (``kvz_multi_prefill``: one split and one combine launch per layer whatever the number of members), every member ending up
        exactly as after its own ``update`` + ``prepare`` + ``attend``.
    Without a packing, first steps (``q_len > 1``) do not go through the batch: they run at batch 1 on each member's own path."""

    _nouns = ("cache batch", "batch", "member", "members", "slack")

    def __init__(self, caches):
        caches = list(caches)
        if not caches:
            raise ops.KvzError("cache batch: needs at least one cache")
        for c in caches:
            if not isinstance(c, EvictCache):
                raise ops.KvzError(f"cache batch: members are pruned EvictCache objects in the slack layout (got {type(c).__name__}: "
                                   "forks share one cache - kvz_fork_attn_append is their launch - and a RetainCache never evicts)")
            if not pruned_slack(c):
                if not (c.pruned and c.info.get("flatten")):
                    raise ops.KvzError("cache batch: a member is not pruned yet (prune() first)")
                raise ops.KvzError("cache batch: a member is in the packed layout (its segments move with every appended token); "
                                   "layout='slack' is what the batched decode step appends to")
        if len({id(c) for c in caches}) != len(caches):
            raise ops.KvzError("cache batch: the same cache twice (two rows of one step would land in one slot)")
        c0 = caches[0]
        for c in caches[1:]:
            if (c.n_heads_kv, c.n_group_kv, c.n_layers, c.dtype) != (c0.n_heads_kv, c0.n_group_kv, c0.n_layers, c0.dtype):
                raise ops.KvzError("cache batch: the members differ in geometry (KV heads, query heads per KV head, layers, dtype): "
                                   f"({c.n_heads_kv}, {c.n_group_kv}, {c.n_layers}, {c.dtype}) vs "
                                   f"({c0.n_heads_kv}, {c0.n_group_kv}, {c0.n_layers}, {c0.dtype})")
            if c.device != c0.device:
                raise ops.KvzError(f"cache batch: the members live on {c0.device} and {c.device}: one launch works on ONE device")
        B = len(caches)
        if (B > ops.MULTI_MAX_CACHES or B * c0.n_heads_kv > ops.MULTI_MAX_SEGMENTS or c0.n_heads_kv > ops.MULTI_MAX_HEADS
                or c0.n_group_kv > ops.MULTI_MAX_GROUP):
            raise ops.KvzError(f"cache batch: {B} caches x {c0.n_heads_kv} KV heads x {c0.n_group_kv} query heads per KV head: one "
                               f"launch takes at most {ops.MULTI_MAX_CACHES} caches, {ops.MULTI_MAX_SEGMENTS} segments (caches x KV "
                               f"heads), {ops.MULTI_MAX_HEADS} KV heads and {ops.MULTI_MAX_GROUP} query heads per KV head")
        self.caches, self.n_caches = caches, B
        self.n_layers, self.n_heads_kv, self.n_group_kv = c0.n_layers, c0.n_heads_kv, c0.n_group_kv
        self.device, self.dtype = c0.device, c0.dtype
        self.pruned, self.get_score, self.layout = True, False, "multi"
        self.active = [True] * B
        self._packed = None
        self._tables = {}   # (members' layout epochs, member order) -> the tables per layer (_table)
        self._ws = None
        self._pws = None

    def get_seq_length(self, layer_idx: Optional[int] = 0) -> int:
        return max(c.get_seq_length(layer_idx) for c in self.caches)

    def _table(self, layer_idx: int, order: Optional[Tuple[int, ...]] = None) -> "ops.MultiTable":
        """The layer's table with the members in ``order`` (None: as the batch lists them, what a decode step takes; the runs of a
        packing lie in the order it names its members).  Built for all layers at an order's first use and kept until a member's
        layout changes, which drops every order's tables: the decode order and a packing order live side by side."""
        key = (tuple([c._layout_epoch for c in self.caches]), order)
        tables = self._tables.get(key)
        if tables is None:
            if any(k[0] != key[0] for k in self._tables) or len(self._tables) > 4:
                self._tables.clear()
            Hkv = self.n_heads_kv
            cs = self.caches if order is None else [self.caches[b] for b in order]
            metas = [c.info["meta_host"] for c in cs]
            tables = self._tables[key] = [ops.MultiTable([c.key_cache[l] for c in cs], [c.value_cache[l] for c in cs],
                                                         [list(m[l][:Hkv]) for m in metas], [list(m[l][Hkv:2 * Hkv]) for m in metas],
                                                         [c.slack for c in cs]) for l in range(self.n_layers)]
        return tables[layer_idx]

    def first_step(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor, layer_idx: int,
                   softmax_scale: Optional[float] = None) -> torch.Tensor:
        """The packed first step of the selected members (``select_packed``): query ``[1, H, T, D]``, key / value ``[1, Hkv, T, D]``
        with ``T = sum(lengths)``, the members' query tokens back to back.  Every member's rows go to its own slack and see only its
        own segments and its own run (bottom-right causal); returns ``[Hkv, T, G, D]``.  Afterwards every member with positions is
        exactly as after its own ``update`` + ``prepare`` + ``attend`` with ``q_len = lengths[i]``."""
        if self._packed is None:
            raise ops.KvzError("cache batch: first_step needs a packing (select_packed): without one, first steps run at batch 1 on "
                               "each cache's own path")
        members, lengths, order, cu = self._packing(query_states)
        T, D = query_states.shape[2], query_states.shape[3]
        if not all(pruned_slack(self.caches[b]) for b in members):
            raise ops.KvzError("cache batch: a member is no longer a pruned slack-layout cache")
        offsets = []
        for b, n in zip(members, lengths):
            c = self.caches[b]
            off = c.info["offset"][layer_idx]
            if n and off + n > c.slack:
                c._grow_slack(off + n)      # (bumps the member's layout epoch: the table below is rebuilt)
            offsets.append(off)
        offsets += [0] * (self.n_caches - len(members))     # (the members that take no part: empty runs at the end)
        table = self._table(layer_idx, tuple(order))
        if self._pws is None or self._pws[0] != (T, D):
            self._pws = ((T, D), ops.multi_prefill_workspace(T, self.n_caches, self.n_heads_kv, self.n_group_kv, D, self.device))
        out = ops.multi_prefill(query_states, cu, table, offsets, key_states, value_states, softmax_scale=softmax_scale,
                                workspace=self._pws[1])
        for b, n, off in zip(members, lengths, offsets):
            if n:
                c = self.caches[b]
                c.info["offset"][layer_idx] = off + n
                if layer_idx == 0:
                    c._seen_tokens += n
        self._packing_done(layer_idx)
        return out

    def update_attend(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor, layer_idx: int,
                      softmax_scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Decode step of all members: query ``[B, H, 1, D]``, key / value ``[B, Hkv, 1, D]`` -> ``[B, Hkv, G, D]``.  Live members get
        their new row appended to their own slack and their bookkeeping advanced as by ``EvictCache.update_attend``; retired ones are
        skipped (their output rows are zero)."""
        B, _, q_len, D = query_states.shape
        if B != self.n_caches or q_len != 1:
            raise ops.KvzError(f"cache batch: a decode step takes [{self.n_caches}, H, 1, D] queries (got batch {B}, {q_len} positions): "
                               "first steps run at batch 1 on each cache's own path")
        offsets = []
        for c, live in zip(self.caches, self.active):
            if not live:
                offsets.append(-1)
                continue
            if not pruned_slack(c):
                raise ops.KvzError("cache batch: a member is no longer a pruned slack-layout cache")
            off = c.info["offset"][layer_idx]
            if off + 1 > c.slack:
                c._grow_slack(off + 1)      # (bumps the member's layout epoch: the table below is rebuilt)
            offsets.append(off)
        table = self._table(layer_idx)
        key_states, value_states = _decode_rows(key_states, value_states)
        if self._ws is None or self._ws[0] != D:
            self._ws = (D, ops.multi_attn_workspace(B, self.n_heads_kv, self.n_group_kv, D, self.device))
        q = query_states.reshape(B, self.n_heads_kv, self.n_group_kv, D).contiguous()
        out = ops.multi_attn_append(q, table, offsets, key_states, value_states, softmax_scale=softmax_scale, workspace=self._ws[1],
                                    out=out)
        for c, off in zip(self.caches, offsets):
            if off >= 0:
                c.info["offset"][layer_idx] = off + 1
                if layer_idx == 0:
                    c._seen_tokens += 1
        return out


class RetainCache(_CacheBase):
    """KV cache that keeps the full KV in memory and subsamples it at every attention call, so that several
    compression ratios can be evaluated from a single prefill (reference attention/kvcache.py:216-347).
    Produces the same flattened tensors as :class:`EvictCache` (the reference's internal cross-check)."""

    def __init__(self, model, evict_range: Tuple[int, int], device=None, dtype=None, reserve: int = 4096,
                 verbose: bool = True, indexed: bool = True):
        super().__init__(model, evict_range, device=device, dtype=dtype, reserve=reserve)
        self.verbose = verbose
        self._cu_head = torch.arange(self.n_heads_kv + 1, dtype=torch.int32, device=self.device)
        # indexed: ``prune`` turns the mask into an index of kept positions (ops.RetainIndex) and decode steps attend through it over
        # the dense store (``update_attend``: no plan, no gather, no host round trip per call); False: every call takes ``prepare``
        self.indexed = bool(indexed)
        self._index: Optional["ops.RetainIndex"] = None
        self._index_valid = None                 # the mask the index was built from (a replaced ``valid`` drops the index)

    # reference: kvcache.py:244-267
    def update(self, key_states: torch.Tensor, value_states: torch.Tensor, layer_idx: int, cache_kwargs=dict()):
        if layer_idx == 0:
            seen_token = (cache_kwargs or {}).get("seen_token", key_states.shape[-2])
            self._seen_tokens += seen_token
        self._dense_append(layer_idx, key_states, value_states)
        return self.key_cache[layer_idx], self.value_cache[layer_idx]

    # reference: kvcache.py:269-276
    def slice(self, seen_token_prev: int):
        assert len(self.key_cache[0].shape) == 4, "Cache at each layer should be 4D tensor"
        self._dense_slice(seen_token_prev)
        self._seen_tokens = seen_token_prev

    # reference: kvcache.py:278-282
    def _mem(self) -> float:
        mem = self.n_layers * self.key_cache[0].numel() * self.key_cache[0].element_size()
        return round(2 * mem / 10**9, 1)

    # reference: kvcache.py:284-298
    def prune(self, ratio: float, level: str = "pair"):
        """Prune the KV cache (fake): only the mask is computed; it is applied before every attention."""
        self._index = self._index_valid = None
        thres, r_ = self._select(ratio, level)
        self.pruned = True
        if self.indexed:
            self._build_index()
        if self.verbose:
            print(f"ratio {r_:.2f} ({level}), threshold {thres:.4f} (evict {self._evicted:.0f} pairs)")
        return thres, r_

    def _build_index(self):
        """Kept positions of every (layer, head) under the current mask: the plan at ``klen = sink + N``, ONE copy of the per-head
        counts to the host, one launch for all layers.  It holds positions, not addresses: growing the dense store leaves it valid."""
        if not self.valid.is_cuda or self.n_heads_kv > 64:   # (the kernel's limit; such a cache keeps the gather route)
            return
        plan = ops.compact_plan(self.valid, self.sink, self.sink + self.ctx_len, slack=0)
        self._index = ops.retain_index(plan)
        self._index_valid = self.valid

    def adopt_dense(self, store_k: List[torch.Tensor], store_v: List[torch.Tensor], filled: int):
        self._index = self._index_valid = None
        super().adopt_dense(store_k, store_v, filled)

    def index_takes(self, query_states: torch.Tensor) -> bool:
        """True when a forward pass with these queries attends through the index: the cache is pruned under the mask the index
        was built from and the kernel takes the shape (batch 1, fp16 / bf16, head dim 64 / 128, few enough query rows per KV head;
        more rows - a long first step - gather and run the multi-row kernel, ``prepare`` + ``attend``)."""
        if not (self.indexed and self.pruned and self._index is not None and self._index_valid is self.valid):
            return False
        bsz, _, q_len, dim = query_states.shape
        if bsz != 1 or not query_states.is_cuda or query_states.dtype not in (torch.float16, torch.bfloat16):
            return False
        return ops._lib.load().kvz_retain_attn_workspace_bytes(self.n_heads_kv, self.n_group_kv, q_len, dim) > 0 and dim in (64, 128)

    def update_attend(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor, layer_idx: int,
                      softmax_scale: Optional[float] = None) -> torch.Tensor:
        """``update`` + ``prepare`` + ``attend`` through the index (``index_takes`` said so): the new rows go into the dense store and
        the queries attend to the kept rows where they lie.  A decode step (one token) is ONE library call that also writes the
        token's row; a few positions are ``update`` followed by one call.  ``_fill``, the ``key_cache`` / ``value_cache`` views and
        ``_seen_tokens`` end up exactly as after ``update``.  Returns ``[Hkv*q_len, G, D]`` like ``attend``: the bits of the gather
        route."""
        bsz, _, q_len, dim = query_states.shape
        ix = self._index
        ws = self._attn_workspace(q_len, dim, query_states.device)
        if q_len == 1 and key_states.stride(-1) == 1 and value_states.stride(-1) == 1:
            if layer_idx == 0:
                self._seen_tokens += 1
            self._flush_append()
            if self._pending:
                self._wait_score(layer_idx)
            f = self._fill[layer_idx]
            sk, sv = self._dense_grow(layer_idx, f + 1)
            out = ops.retain_attn_append(query_states.reshape(-1, self.n_group_kv, dim), sk, sv, key_states, value_states, ix.idx,
                                         ix.meta_host[layer_idx], ix.ctx_end, f, softmax_scale=softmax_scale, workspace=ws)
            self._dense_commit(layer_idx, f + 1)
            return out
        self.update(key_states, value_states, layer_idx)
        query_states = query_states.view(bsz, self.n_heads_kv, self.n_group_kv, q_len, dim)
        query_states = query_states.transpose(2, 3).contiguous().view(-1, self.n_group_kv, dim)
        return ops.retain_attn(query_states, self._store_k[layer_idx], self._store_v[layer_idx], ix.idx, ix.meta_host[layer_idx],
                               ix.ctx_end, self._fill[layer_idx], q_len, causal=True, softmax_scale=softmax_scale, workspace=ws)

    # reference: kvcache.py:312-347
    def prepare(self, query_states: torch.Tensor, key_states: torch.Tensor, value_states: torch.Tensor,
                layer_idx: int):
        bsz, n_heads_q, q_len, dim = query_states.shape
        klen = key_states.size(2)
        query_states = query_states.view(bsz, self.n_heads_kv, self.n_group_kv, q_len, dim)
        query_states = query_states.transpose(2, 3).contiguous().view(-1, self.n_group_kv, dim)
        cu_seqlens_q = q_len * self._cu_head

        plan = ops.compact_plan(self.valid[layer_idx:layer_idx + 1], self.sink, klen, slack=0)
        total = int(plan.cu_len_k[0, -1])  # host sync, as the reference's boolean indexing
        if plan.heads:  # head-level mask (one byte per head): the batched entry point takes it
            ks, vs = ops.compact_layers([key_states], [value_states], plan, [total])
            k_flat, v_flat = ks[0], vs[0]
        else:
            k_flat, v_flat = ops.compact_layer(key_states, value_states, plan, 0, total)
        info = {
            "cu_len_q": cu_seqlens_q,
            "cu_len_k": plan.cu_len_k[0],
            "max_len_q": q_len,
            "max_len_k": int(plan.max_len_k[0]),
            "k_start": plan.seg_start[0],
            "k_len": plan.len_k[0],
            "k_len_offset": 0,
        }
        return query_states, k_flat.view(-1, 1, dim), v_flat.view(-1, 1, dim), info

    attend = EvictCache.attend
    _workspace, _attn_workspace = EvictCache._workspace, EvictCache._attn_workspace
    _attn_ws = None
