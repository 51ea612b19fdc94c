"""ModelKVzip — the model-level API of the reference (reference model/wrapper.py:61-306), same method names and
argument meaning: ``prefill / scoring / self_task / generate / apply_template / __call__ / _prob``.

    model = ModelKVzip("Qwen/Qwen2.5-7B-Instruct-1M")     # or ModelKVzip(hf_model, tokenizer=tok)
    kv = model.prefill(context, load_score=False)          # prefill KV cache + importance scoring
    kv.prune(ratio=0.3)                                     # eviction (score -> select -> compact on the GPU)
    answer = model.generate(query, kv=kv, update_cache=False)

What differs from the reference (deliberately):
  * the model may be passed as an object (random-init models from a config work: there is no network here);
  * token ids can be used everywhere text is accepted, so the eviction path runs without a tokenizer;
  * generation is a small greedy loop over the patched HF decoder (the reference calls ``model.generate`` of
    transformers 4.51.3, whose cache plumbing changed in 5.x); semantics kept: greedy, ``max_new_tokens``,
    the cache is sliced back to the context unless ``update_cache=True``;
  * head-level scores (``load_score=True``) are read from ``head_score_dir`` (the reference hard-codes
    ./utils/head_score/, model/wrapper.py:40-58).
"""
from __future__ import annotations

import glob
import os
from typing import List, Optional, Tuple, Union

import torch

from . import ops
from .kvcache import CacheBatch, EvictCache, ForkedCache, RetainCache, pruned_slack
from .monkeypatch import replace_attn
from .ops import KvzError
from .template import template


def chunk_fn(ctx_ids: torch.Tensor, chunk_size: int) -> List[torch.Tensor]:
    """Split ``[1, n]`` token ids into chunks of ``chunk_size`` (reference model/wrapper.py:18-37)."""
    n = ctx_ids.shape[1]
    if n <= chunk_size:
        return [ctx_ids]
    return [ctx_ids[:, s:s + chunk_size] for s in range(0, n, chunk_size)]


def head_score_name(model_name: str) -> str:
    """File-name stem of a model's head-score files (reference model/wrapper.py:41-46)."""
    for prefix, short in (("Qwen2.5-7B", "qwen2.5-7b"), ("Qwen2.5-14B", "qwen2.5-14b"), ("Llama-3.1-8B", "llama3.1-8b")):
        if model_name.startswith(prefix):
            return short
    return model_name


def load_head_score(model_name: str, ctx_len: int, head_score_dir: str, device) -> torch.Tensor:
    """Head-level scores expanded over the context: ``[L, 1, Hkv, ctx_len]`` (reference model/wrapper.py:40-58).
    The expansion is a stride-0 VIEW of the ``[L, Hkv]`` maxima: ``prune`` recognises it and selects / compacts whole
    heads without ever materialising anything of size ``ctx_len``."""
    name = head_score_name(model_name)
    paths = sorted(glob.glob(os.path.join(head_score_dir, f"{name}-*.pt")))
    if not paths:
        raise FileNotFoundError(f"no head-score file {name}-*.pt under {head_score_dir}")
    attn = torch.stack([torch.load(p, map_location="cpu").squeeze() for p in paths], dim=0).amax(0).to(device)
    return attn.unsqueeze(-1).expand(-1, -1, ctx_len).unsqueeze(1)


def _on_model_device(fn):
    """Run a ModelKVzip method with the model's GPU as the current device: the library launches on the CURRENT HIP device, and a
    model that lives on cuda:1 while cuda:0 is current must work the same way (side streams, events, workspaces of the cache)."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        dev = self.device   # (always a GPU: __init__ refuses anything else)
        with torch.cuda.device(dev):
            return fn(self, *args, **kwargs)
    return wrapped


class ModelKVzip:

    def __init__(self, model: Union[str, torch.nn.Module], kv_type: str = "evict", tokenizer=None,
                 name: Optional[str] = None, head_score_dir: str = "./utils/head_score", max_new_tokens: int = 512,
                 eos_token_id: Optional[Union[int, List[int]]] = None, cache_kwargs: Optional[dict] = None):
        if isinstance(model, str):  # reference model/load.py:58-64 (needs the HF hub or a local path)
            from transformers import AutoModelForCausalLM, AutoTokenizer
            replace_attn(model)
            name = name or model.split("/")[-1]
            tokenizer = tokenizer or AutoTokenizer.from_pretrained(model)
            # ONE device: a cache object (side streams, events, workspaces) lives on one GPU, and the multi-GPU scheme of this path is
            # one context per GPU (kvzip_amd/dist.py), not one model sharded over several
            if not torch.cuda.is_available():
                raise KvzError("ModelKVzip needs a GPU: the hot path (dense and post-prune attention, scoring, selection, compaction) "
                               "runs on the library's HIP kernels only, there is no CPU implementation")
            dev = f"cuda:{torch.cuda.current_device()}"
            model = AutoModelForCausalLM.from_pretrained(model, torch_dtype="auto", device_map=dev).eval()
        else:
            replace_attn(name or type(model).__name__)
        self.model, self.tokenizer = model, tokenizer
        devices = {p.device for p in model.parameters()}
        if len(devices) > 1:
            raise ValueError(f"the model is sharded over {sorted(map(str, devices))}: ModelKVzip needs it on ONE device (one context "
                             "per GPU is the multi-GPU scheme of this path, kvzip_amd/dist.py)")
        self.name = name or type(model).__name__
        self.dtype = next(model.parameters()).dtype
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":   # (fail HERE, not at the first forward inside kvzip_amd.attn)
            raise KvzError(f"ModelKVzip: the model lives on {self.device}; the product path has no CPU implementation - move it to the GPU "
                           "(model.to('cuda')) before wrapping it")
        self.config = model.config
        self.config._attn_implementation = "kvzip_hip"  # dense path through kvzip_amd.attn, no HF mask construction
        self.kv_type = kv_type
        # f2: scoring passes can take the row statistics of the scores from the forward's own attention kernel (one QK^T over the
        # window instead of two).  Built, parity-tested - and OFF by default: the row-statistics pass is bound by its VALU rounding
        # chain, not by the matrix cores, so sharing the QK^T saves nothing, and inside the forward that chain sits on the critical
        # path (+17 % on a 2 026 x 35 k forward, profiles/r3_flash_probe.txt) instead of on a side stream beside the MLP GEMMs
        self.fuse_forward_score = False
        self.head_score_dir = head_score_dir
        self.cache_kwargs = dict(cache_kwargs or {})
        # the reference's generation settings (model/wrapper.py:81-94): greedy by default, the sampling knobs of HF generate under
        # the same names; Qwen3 stops at <|im_end|> = 151645 like there
        self.gen_kwargs = {"do_sample": False, "temperature": 1.0, "top_p": 1, "top_k": None, "max_new_tokens": max_new_tokens}
        if eos_token_id is None and getattr(self.config, "model_type", "") == "qwen3":
            eos_token_id = 151645
        if eos_token_id is None:
            eos_token_id = getattr(model.generation_config, "eos_token_id", None) if hasattr(model, "generation_config") else None
        if eos_token_id is not None:
            self.gen_kwargs["eos_token_id"] = eos_token_id
        # branches of one forked decode wave (generate_batch), besides the kernel's own limit of 64 // G: the measured per-token cost
        # keeps falling up to that limit (profiles/fork_decode_ab.txt), so the default does not cap below it
        self.fork_max_branches = 16
        # generate_batch: the first steps of all branches of a wave as ONE packed forward pass (kvcache.ForkedCache.select_packed:
        # the shared context and the model's weights are read once per wave instead of once per query); False: one forward per branch
        self.fork_packed_first = True
        self.multi_packed_first = True   # generate_multi: the first steps of a wave as ONE packed forward pass (CacheBatch.first_step)
        self.multi_max_caches = 16   # caches of one batched decode wave (generate_multi), besides the kernel's own limit of 128 // Hkv
        self.last_beam_hypotheses: List[Tuple[float, List[int]]] = []   # generate_beam: (score, generated tokens) of its hypotheses
        self.sample_generator: Optional[torch.Generator] = None   # seed source of do_sample=True (None: torch's global generator)
        self.sys_prompt_ids = torch.zeros((1, 0), dtype=torch.long, device=self.device)
        self.postfix_ids = torch.zeros((1, 0), dtype=torch.long, device=self.device)
        if tokenizer is not None:
            self.set_chat_template()

    # ---- text <-> ids (reference model/wrapper.py:99-118) -----------------------------------------------
    def encode(self, text: str) -> torch.Tensor:
        if self.tokenizer is None:
            raise ValueError("no tokenizer: pass token-id tensors instead of text")
        return self.tokenizer.encode(text, add_special_tokens=False, return_tensors="pt").to(self.device)

    def _ids(self, query: Union[str, torch.Tensor]) -> torch.Tensor:
        """Text or token ids -> ``[1, n]`` ids on the model's device."""
        return self.encode(query) if isinstance(query, str) else query.to(self.device)

    def decode(self, input_ids: torch.Tensor) -> str:
        if input_ids.dim() == 2:
            input_ids = input_ids[0]
        if self.tokenizer is None:
            return " ".join(str(int(t)) for t in input_ids)
        return self.tokenizer.decode(input_ids)

    def set_chat_template(self, task: str = "qa"):
        prefix, postfix = template(self.name, task)
        self.sys_prompt_ids, self.postfix_ids = self.encode(prefix), self.encode(postfix)

    def set_prompt_ids(self, sys_prompt_ids: torch.Tensor, postfix_ids: torch.Tensor):
        """Tokenizer-free variant of ``set_chat_template``."""
        self.sys_prompt_ids, self.postfix_ids = sys_prompt_ids.to(self.device), postfix_ids.to(self.device)

    def apply_template(self, query: Union[str, torch.Tensor]) -> torch.Tensor:
        q_ids = self.encode(f"\n\n{query.strip()}") if isinstance(query, str) else query.to(self.device)
        return torch.cat([q_ids, self.postfix_ids], dim=1)

    # ---- forward (reference model/wrapper.py:120-146) ---------------------------------------------------------
    @_on_model_device
    @torch.inference_mode()
    def __call__(self, input_ids: torch.Tensor, kv, update_cache: bool = False, return_logits: bool = False,
                 *args, **kwargs):
        """Transformer forward pass.  By default the KV of ``input_ids`` is NOT kept (``update_cache=False``)."""
        seen_token_prev = kv._seen_tokens
        if return_logits:
            outputs = self.model(input_ids, past_key_values=kv, use_cache=True, *args, **kwargs)
        else:
            _ = self.model.model(input_ids, past_key_values=kv, use_cache=True, *args, **kwargs)
            outputs = None
        if not update_cache:
            kv.slice(seen_token_prev)
        return outputs

    def _init_kv(self, kv=None, evict_range: Tuple[int, int] = (0, 0)):
        if kv is None:
            if self.kv_type == "retain":
                kv = RetainCache(self.model, evict_range, **self.cache_kwargs)
            elif self.kv_type == "evict":
                kv = EvictCache(self.model, evict_range, **self.cache_kwargs)
            else:
                raise NotImplementedError(f"type {self.kv_type} is not implemented on this path "
                                          "(int4static / hybrid_static are retain-only in the reference)")
        return kv

    # ---- prefill + scoring (reference model/wrapper.py:169-249) ------------------------------------------------
    @_on_model_device
    @torch.inference_mode()
    def prefill(self, ctx_ids: Union[str, torch.Tensor], prefill_chunk_size: int = 16000, load_score: bool = False,
                do_score: bool = True):
        """Chunked prefill of the KV cache, then KV importance scoring."""
        ctx_ids = self._ids(ctx_ids)
        prefill_ids = torch.cat([self.sys_prompt_ids, ctx_ids], dim=1)
        evict_range = (self.sys_prompt_ids.shape[1], prefill_ids.shape[1])
        kv = self._init_kv(evict_range=evict_range)  # the system prompt is never evicted
        kv.ctx_ids = ctx_ids
        kv.prefill_ids = prefill_ids
        for input_ids in chunk_fn(prefill_ids, prefill_chunk_size):
            self.__call__(input_ids, kv, update_cache=True)
        if do_score:
            self.scoring(kv, ctx_ids, load_score=load_score)
        return kv

    def self_task(self, ctx_ids: torch.Tensor, chunk_size: int = 2000, prev_postfix_size: int = 8,
                  repeat_prompt_ids: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """Chunked "repeat the context" inputs: list of (chunk ids, repeat prompt ++ postfix ++ chunk ids)."""
        chunked = chunk_fn(ctx_ids.to(self.device), chunk_size)
        if repeat_prompt_ids is None:
            first = self.encode("\n\nRepeat the previous context exactly.")
            later = self.encode("\n\nRepeat the part of the previous context exactly, starting with ")
        else:
            first, later = (t.to(self.device) for t in repeat_prompt_ids)
        inputs = []
        for i, a_ids in enumerate(chunked):
            if i == 0:
                q_ids = first
            else:
                q_ids = torch.cat([later, chunked[i - 1][:, -prev_postfix_size:]], dim=1)
            inputs.append((a_ids, torch.cat([q_ids, self.postfix_ids, a_ids], dim=1)))
        return inputs

    @_on_model_device
    @torch.inference_mode()
    def scoring(self, kv, ctx_ids: torch.Tensor, load_score: bool = False, chunk_size: int = 2000,
                repeat_prompt_ids=None):
        """KV importance scoring (fills ``kv.score``)."""
        if not load_score:
            kv.init_score()
            fused = hasattr(kv, "fuse_update_score")
            if fused:
                kv.fuse_update_score = True  # the forward pass is kvzip_amd.attn: update() is always followed by _get_score()
                kv.fuse_forward_score = self.fuse_forward_score  # ... and its attention kernel emits the row statistics (f2)
            start_idx_tmp = kv.start_idx
            kv.end_idx = 0
            try:
                for prefill_ids_p, repeat_ids_p in self.self_task(ctx_ids, chunk_size=chunk_size,
                                                                  repeat_prompt_ids=repeat_prompt_ids):
                    kv.end_idx = kv.start_idx + prefill_ids_p.shape[1]      # window of this chunk
                    self.__call__(repeat_ids_p, kv, update_cache=False)     # the patched attention calls kv._get_score
                    kv.start_idx = kv.end_idx
            finally:
                # also when a forward pass raised (out of memory ...): the cache must not stay in the mode in which update()
                # returns views whose new rows are still to be written, nor keep the chunk's K,V pinned
                kv.start_idx = start_idx_tmp
                if fused:
                    kv.fuse_update_score = False
                    kv.fuse_forward_score = False
                    kv._flush_append()
            assert kv.score[0].shape[-1] == kv.ctx_len
        else:
            kv.score = load_head_score(self.name, kv.ctx_len, self.head_score_dir, self.device)
        kv.get_score = False

    @property
    def eos_token_ids(self) -> List[int]:
        e = self.gen_kwargs.get("eos_token_id")
        return [e] if isinstance(e, int) else list(e or [])

    @staticmethod
    def next_token(logits: torch.Tensor, gen_kwargs: dict, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """Next token ``[b, 1]`` from last-position logits ``[b, V]`` under the reference's ``gen_kwargs`` (model/wrapper.py:81-87,
        passed to HF ``generate`` there): ``do_sample=False`` -> argmax; otherwise temperature, then top-k, then top-p (nucleus: the
        smallest set of most probable tokens whose mass reaches ``top_p``, at least one token), then one multinomial draw - the
        order and the semantics of transformers' logits warpers."""
        if not gen_kwargs.get("do_sample", False):
            return logits.argmax(-1, keepdim=True)
        x = logits.float()
        t = gen_kwargs.get("temperature", 1.0)
        if t is not None and t != 1.0:
            x = x / float(t)
        k = gen_kwargs.get("top_k")
        if k:
            kth = torch.topk(x, min(int(k), x.shape[-1]), dim=-1).values[..., -1:]
            x = x.masked_fill(x < kth, float("-inf"))
        p = gen_kwargs.get("top_p", 1)
        if p is not None and p < 1:
            sx, si = torch.sort(x, dim=-1, descending=False)
            cum = torch.softmax(sx, dim=-1).cumsum(-1)
            drop = cum <= (1 - float(p))          # the low-probability tail whose mass stays below 1 - top_p
            drop[..., -1:] = False                # (at least the most probable token survives)
            x = x.masked_fill(torch.zeros_like(drop).scatter(-1, si, drop), float("-inf"))
        return torch.multinomial(torch.softmax(x, dim=-1), 1, generator=generator)

    # ---- generation (reference model/wrapper.py:251-284) ---------------------------------------------------------
    @_on_model_device
    @torch.inference_mode()
    def generate(self, query: Union[str, torch.Tensor], kv=None, update_cache: bool = False,
                 return_ids: bool = False):
        """Response to ``query`` under ``self.gen_kwargs`` (the reference's knobs, model/wrapper.py:81-94: greedy by default;
        ``do_sample / temperature / top_k / top_p / max_new_tokens / eos_token_id`` as HF ``generate`` takes them there).  The
        reference hands the loop to ``model.generate(input_ids, past_key_values=kv, **gen_kwargs)`` (model/wrapper.py:276); the
        token loop lives here because the cache object is not a ``transformers.Cache`` subclass in transformers 5.x - same tokens
        for the same knobs, and like there the prompt is only what is new (HF slices ``input_ids[:, -new:]`` off the full
        sequence).  The KV of the query and of the answer is evicted afterwards (``kv.slice``) unless ``update_cache=True``
        (multi-turn)."""
        kv = self._init_kv(kv=kv)
        seen_token_prev = kv._seen_tokens
        input_ids = self._ids(query)
        out_ids = []
        cur = input_ids
        for _ in range(self.gen_kwargs["max_new_tokens"]):
            logits = self.model(cur, past_key_values=kv, use_cache=True).logits[:, -1]
            nxt = self.next_token(logits, self.gen_kwargs, self.sample_generator)
            out_ids.append(nxt)
            if self.eos_token_ids and int(nxt) in self.eos_token_ids:
                break
            cur = nxt
        # the reference drops the last generated token (model/wrapper.py:277: output[:, len(input_ids):-1]): it is the
        # terminating EOS (or the token that hit max_new_tokens) and its KV was never written to the cache
        a_ids = torch.cat(out_ids, dim=1)[:, :-1]
        self._end_turn(kv, update_cache, seen_token_prev, input_ids, a_ids)
        return a_ids if return_ids else self.decode(a_ids)

    @staticmethod
    def _end_turn(kv, update_cache: bool, seen_prev: Optional[int], q_ids: torch.Tensor, a_ids: torch.Tensor) -> None:
        """How a turn leaves its cache: sliced back to the ``seen_prev`` tokens it held before, or (``update_cache``, multi-turn)
        keeping the rows of query and answer, with ``prefill_ids`` grown by them."""
        if not update_cache:
            kv.slice(seen_prev)
        elif kv.prefill_ids is not None:
            kv.prefill_ids = torch.cat([kv.prefill_ids, q_ids, a_ids], dim=1)

    def _group(self) -> int:
        """Query heads per KV head (G)."""
        return self.config.num_attention_heads // self.config.num_key_value_heads

    def _fork_wave(self) -> int:
        """Branches of one forked decode wave: ``fork_max_branches`` within what one launch takes."""
        return max(1, min(self.fork_max_branches, ops.FORK_MAX_BRANCHES, ops.FORK_MAX_ROWS // self._group()))

    def _draft_len(self, num_draft: Optional[int] = None) -> int:
        """Drafted tokens per verify step (the step runs t = 1 + draft positions).  The default keeps t*G <= 32 query rows per KV
        head - one block per work item, where the forked decode's step time holds - and a request is capped at t*G <= 64,
        the kernel's limit.  Both come from the forked-decode table, not from a measurement of the verify kernel: a shape that
        tools/spec_decode_bench.py flags as slower than the existing path gets its rule HERE."""
        G = self._group()
        cap = max(0, 64 // G - 1)
        if num_draft is None:
            return max(0, 32 // G - 1)
        return max(0, min(int(num_draft), cap))

    @_on_model_device
    @torch.inference_mode()
    def generate_speculative(self, query: Union[str, torch.Tensor], kv, draft=None, num_draft: Optional[int] = None,
                             update_cache: bool = False, return_ids: bool = False, return_stats: bool = False, tree: bool = False):
        """``generate`` by draft-and-verify on a pruned slack-layout cache, greedy (no reference counterpart).  After the query's
        first step every further step asks the drafter for up to ``num_draft`` ids (``draft(history_ids, n)`` if given, else prompt
        lookup over ``kv.prefill_ids ++ query ++ answer``, ``draft.lookup_draft``), runs ``[last token] ++ draft`` through the model
        in ONE forward pass whose attention reads the kept rows once (``EvictCache.verify_attend``), keeps the longest prefix of the
        draft the model agrees with plus the model's own token behind it, and takes the rejected positions back (``kv.rewind``).  An
        empty draft is a plain decode step.  Same tokens as ``generate`` up to the summation order of the attention (an argmax may
        tie); the answer ends at the first EOS or at ``max_new_tokens``, its last token is dropped and the cache is left as
        ``generate`` leaves it.  ``return_stats``: also ``{"steps", "tokens", "drafted", "accepted"}`` (forward passes after the query's,
        tokens they produced, ids drafted, ids accepted).  End-to-end gain depends on the drafter's hit rate.

        ``tree=True``: a step verifies a TREE of candidates, so that several continuations share the forward pass.  The drafter is
        ``draft(history_ids, n) -> (ids, parents)`` (default ``draft.lookup_tree``): up to n nodes behind the root, the last token;
        ``parents[i]`` is the node ``ids[i]`` (node i + 1) continues, 0 being the root, parents before children.  Node i runs at
        position ``seen + depth(i)`` and attends to its ancestors among the new rows (``kv.verifying(tree=...)``);
        ``draft.accept_tree_greedy`` picks the path the model agrees with, ``kv.keep_path`` keeps its rows.  The node budget is
        ``num_draft``'s (t*G <= 32 query rows per KV head by default, at most 64).  Stats also carry ``"nodes"``, the positions the
        verify steps ran (root included); ``"drafted"`` counts the nodes behind the roots, ``"accepted"`` those on accepted paths."""
        from .draft import accept_greedy, accept_tree_greedy, lookup_draft, lookup_tree
        if self.gen_kwargs.get("do_sample", False):
            raise ValueError("generate_speculative is greedy: do_sample=True needs a distribution-preserving acceptance rule, use generate")
        if not (isinstance(kv, EvictCache) and pruned_slack(kv)):
            raise ValueError("generate_speculative needs a pruned slack-layout EvictCache (the verify step appends to and rewinds the "
                             "slack behind the kept rows): use generate for a dense or packed-layout cache")
        seen_token_prev = kv._seen_tokens
        input_ids = self._ids(query)
        max_new = self.gen_kwargs["max_new_tokens"]
        eos = self.eos_token_ids
        n_draft = self._draft_len(num_draft)
        drafter = draft if draft is not None else (lookup_tree if tree else lookup_draft)
        prior = [kv.prefill_ids[0]] if getattr(kv, "prefill_ids", None) is not None else []
        history = torch.cat(prior + [input_ids[0]])
        stats = {"steps": 0, "tokens": 0, "drafted": 0, "accepted": 0}
        if tree:
            stats["nodes"] = 0
        logits = self.model(input_ids, past_key_values=kv, use_cache=True).logits[:, -1]
        out = [int(logits.argmax(-1))]          # invariant: the cache holds the query and out[:-1]
        while len(out) < max_new and out[-1] not in eos:
            room = max_new - len(out)
            last = torch.tensor([out[-1]], dtype=torch.long, device=self.device)
            history = torch.cat([history, last])
            d_ids = history[:0]
            if n_draft > 0 and room > 1 and tree:
                d_ids, parents = drafter(history, min(n_draft, room - 1))
                d_ids = torch.as_tensor(d_ids, dtype=torch.long).reshape(-1)[:min(n_draft, room - 1)].to(self.device)
                parents = [int(x) for x in parents][:int(d_ids.shape[0])]     # (parents precede children: a prefix is a tree)
            elif n_draft > 0 and room > 1:
                d_ids = drafter(history, min(n_draft, room - 1)).reshape(-1)[:min(n_draft, room - 1)].to(self.device)
            d = int(d_ids.shape[0])
            stats["steps"] += 1
            stats["drafted"] += d
            if d == 0:      # nothing to verify: the plain decode step
                out.append(int(self.model(last[None], past_key_values=kv, use_cache=True).logits[:, -1].argmax(-1)))
                stats["tokens"] += 1
                continue
            cur = torch.cat([last, d_ids])[None]
            if tree:
                depth = [0]
                for par in parents:             # (node i + 1 continues node parents[i]; ancestor_masks checks the order)
                    depth.append(depth[par] + 1 if 0 <= par < len(depth) else 0)
                pos = (kv._seen_tokens + torch.tensor(depth, device=self.device))[None]
                with kv.verifying(tree=[-1] + parents):
                    argmax = self.model(cur, past_key_values=kv, use_cache=True, position_ids=pos).logits[0].argmax(-1)
                argmax = argmax.tolist()
                path = accept_tree_greedy(d_ids, parents, argmax)
                ids_l = d_ids.tolist()
                new = [ids_l[i - 1] for i in path[1:]] + [argmax[path[-1]]]
                stats["accepted"] += len(path) - 1
                stats["nodes"] += d + 1
                for j, tok in enumerate(new):   # an EOS on the path ends the answer there: the nodes behind it are not kept
                    if tok in eos:
                        path, new = path[:j + 1], new[:j + 1]
                        break
                kv.keep_path(path, d + 1)       # the cache holds `last` and the ids of the path
                stats["tokens"] += len(new)
                out += new
                history = torch.cat([history, torch.tensor(new[:-1], dtype=torch.long, device=history.device)])
                continue
            pos = torch.arange(kv._seen_tokens, kv._seen_tokens + d + 1, device=self.device)[None]
            with kv.verifying():
                argmax = self.model(cur, past_key_values=kv, use_cache=True, position_ids=pos).logits[0].argmax(-1)
            a = accept_greedy(d_ids, argmax)
            new = d_ids[:a].tolist() + [int(argmax[a])]
            kv.rewind(d - a)                    # the cache holds `last` and the accepted ids
            stats["accepted"] += a
            for j, tok in enumerate(new):       # an EOS inside the accepted run ends the answer there
                if tok in eos:
                    kv.rewind(a - j)            # (the rows of the ids behind it, and its own, are not part of what generate leaves)
                    new = new[:j + 1]
                    break
            stats["tokens"] += len(new)
            out += new
            history = torch.cat([history, torch.tensor(new[:-1], dtype=torch.long, device=history.device)])
        a_ids = torch.tensor(out[:-1], dtype=torch.long, device=self.device)[None]
        self._end_turn(kv, update_cache, seen_token_prev, input_ids, a_ids)
        res = a_ids if return_ids else self.decode(a_ids)
        return (res, stats) if return_stats else res

    @_on_model_device
    @torch.inference_mode()
    def generate_batch(self, queries, kv, return_ids: bool = False, keep: Optional[int] = None) -> list:
        """Responses to several queries over ONE pruned cache, decoded together (no reference counterpart: the reference answers the
        queries of a context one after the other, eval.py).  Every query becomes a branch of ``kv.fork(...)``: the first steps (the
        query tokens) of all branches of a wave run as ONE packed forward pass (``fork_packed_first``, the default; ``False``: one
        forward per branch at batch 1), then all live branches decode in one batch whose attention reads the shared context once per
        step.  Same knobs as ``generate`` (``gen_kwargs``; the last token of every answer is dropped as there); a branch stops at EOS
        or ``max_new_tokens`` while the others go on.  More queries than one launch takes (``64 // G`` branches, at most 16) run in
        waves.  ``kv`` is left exactly as it was: nothing is appended to it, so there is nothing to slice.  ``keep=i`` is this path's
        ``update_cache=True``: the cache afterwards holds query i and its answer as after ``generate(queries[i], kv,
        update_cache=True)`` - branch i's rows are appended to the base (``ForkedCache.commit``) and ``prefill_ids`` grows - so that a
        multi-turn conversation goes on from the kept branch; only offered when all queries fit one wave (``KvzError`` otherwise).
        Answers agree with ``generate`` up to the summation order of the attention (an argmax may tie)."""
        ids = [self._ids(q) for q in queries]
        wave = self._fork_wave()
        if keep is not None:
            if not 0 <= int(keep) < len(ids):
                raise KvzError(f"generate_batch: keep={keep} names none of the {len(ids)} queries")
            if len(ids) > wave:
                raise KvzError(f"generate_batch: keep= is offered when all queries fit one wave ({wave} branches here: 64 // G, at most "
                               f"{self.fork_max_branches}); got {len(ids)} queries")
        answers: list = []
        for w0 in range(0, len(ids), wave):
            answers += self._generate_wave(ids[w0:w0 + wave], kv, keep=keep)
        return answers if return_ids else [self.decode(a) for a in answers]

    def _packs_first_steps(self, lengths: List[int]) -> bool:
        """Whether a wave of queries of these lengths takes the packed first step.  Every wave of two or more does: packed was faster
        than one pass per branch at every measured shape (2-9 queries of 16-160 tokens, 1.5-6.1 x; profiles/fork_prefill_ab.txt,
        DESIGN 3.10), so there is no shape rule - one would go HERE.  (An empty query has no last position to take a token from: it
        goes to the per-branch loop, which fails on it as it always did.)"""
        return bool(self.fork_packed_first) and all(n > 0 for n in lengths)

    def _decode_slots(self, cache, first_logits: List[torch.Tensor], first_pos: List[int]) -> List[torch.Tensor]:
        """The batched token loop of ``generate_batch / generate_samples / generate_multi``: slot b of ``cache`` (a ``ForkedCache`` or
        a ``CacheBatch``) has run its first step, which left the logits ``first_logits[b]`` (``[1, V]``) and the next position
        ``first_pos[b]``.  Every slot takes its first token, in slot order; then one forward pass per step gives every live slot
        one more, the draws again in slot order.  A slot is retired (``cache.retire``) at EOS or at ``max_new_tokens`` while the
        others go on.  -> the answers ``[1, n_b]`` per slot, the last token dropped (see ``generate``)."""
        B = len(first_logits)
        max_new, eos = self.gen_kwargs["max_new_tokens"], self.eos_token_ids
        out_ids: List[List[torch.Tensor]] = [[] for _ in range(B)]
        cur = torch.zeros((B, 1), dtype=torch.long, device=self.device)
        pos = torch.tensor(first_pos, dtype=torch.long, device=self.device).view(B, 1)
        live = [True] * B

        def take(b, logits):   # the token slot b produces from its logits; retire the slot at EOS / the token budget
            nxt = self.next_token(logits, self.gen_kwargs, self.sample_generator)
            out_ids[b].append(nxt)
            cur[b] = nxt[0]
            if (eos and int(nxt) in eos) or len(out_ids[b]) >= max_new:
                live[b] = False
                cache.retire(b)

        for b in range(B):
            take(b, first_logits[b])
        while any(live):    # one token for every live slot per step
            logits = self.model(cur, past_key_values=cache, use_cache=True, position_ids=pos).logits[:, -1]
            pos += 1
            for b in range(B):
                if live[b]:
                    take(b, logits[b:b + 1])
        return [torch.cat(o, dim=1)[:, :-1] for o in out_ids]

    def _packed_first(self, cache, ids: List[torch.Tensor], starts: List[int]) -> Tuple[List[torch.Tensor], List[int]]:
        """The first steps of all slots of ``cache`` in ONE forward pass: the queries back to back, query b at the positions from
        ``starts[b]`` on.  -> what ``_decode_slots`` takes: every slot's logits at its last packed position, and its next position."""
        lens = [x.shape[1] for x in ids]
        cache.select_packed(list(range(len(ids))), lens)
        p = torch.cat([torch.arange(s, s + n, device=self.device) for s, n in zip(starts, lens)]).unsqueeze(0)
        logits = self.model(torch.cat(ids, dim=1), past_key_values=cache, use_cache=True, position_ids=p).logits
        ends = [sum(lens[:b + 1]) for b in range(len(ids))]
        return [logits[:, e - 1] for e in ends], [s + n for s, n in zip(starts, lens)]

    def _generate_wave(self, ids: List[torch.Tensor], kv, keep: Optional[int] = None) -> List[torch.Tensor]:
        B = len(ids)
        fork = kv.fork(B, tail_capacity=max(x.shape[1] for x in ids) + self.gen_kwargs["max_new_tokens"])
        base_len = kv.get_seq_length()
        if B >= 2 and self._packs_first_steps([x.shape[1] for x in ids]):
            first, pos = self._packed_first(fork, ids, [base_len] * B)
        else:
            first, pos = [], []
            for b in range(B):  # first step of every branch: its query, at batch 1
                fork.select_branch(b)
                n = ids[b].shape[1]
                p = torch.arange(base_len, base_len + n, device=self.device).unsqueeze(0)
                # (a copy of the one row: the logits of the whole query need not live until the last branch has run)
                first.append(self.model(ids[b], past_key_values=fork, use_cache=True, position_ids=p).logits[:, -1].clone())
                pos.append(base_len + n)
        answers = self._decode_slots(fork, first, pos)
        if keep is not None:   # the kept branch's tail - its query rows and the rows of its answer - becomes part of the base cache
            fork.commit(keep)
            self._end_turn(kv, True, None, ids[keep], answers[keep])
        return answers

    def _fork_limit(self, who: str, n: int) -> None:
        G = self._group()
        if n < 1 or n > ops.FORK_MAX_BRANCHES or n * G > ops.FORK_MAX_ROWS:
            raise KvzError(f"{who}: {n} branches x {G} query heads per KV head: one forked decode launch takes at most "
                           f"{ops.FORK_MAX_ROWS} query rows per KV head (branches x G) and at most {ops.FORK_MAX_BRANCHES} branches")

    @_on_model_device
    @torch.inference_mode()
    def generate_beam(self, query: Union[str, torch.Tensor], kv, num_beams: int = 4, length_penalty: float = 1.0,
                      update_cache: bool = False, return_ids: bool = False, num_return: int = 1):
        """Beam search over ONE pruned cache (no reference counterpart: the reference hands ``num_beams`` to HF ``generate``, which
        replicates the whole cache per beam).  The query's first step runs ONCE on the base cache on the sequential path, as
        ``generate``'s does; then the beams are the branches of ``kv.fork(num_beams)``, which sees the query rows as shared, so a
        tail holds generated tokens only and a step reads the context once for all beams.  Per step: fp32 ``log_softmax`` of every live
        beam's logits, the top ``2 * num_beams`` of the ``beams x V`` continuations by summed log-probability, walked best first - a
        continuation that ends in EOS becomes a finished hypothesis if it ranks among the first ``num_beams``, the first ``num_beams``
        others are the next beams - then ``fork.reorder(parents)`` moves the tails (one copy per dropped beam).  A hypothesis scores
        ``sum_logprob / len ** length_penalty``, ``len`` counting every generated token, the last one included.  The search stops when
        ``num_beams`` hypotheses are finished and no live beam can still beat the worst of them (for ``length_penalty > 0`` the bound
        of a live beam is its sum over ``max_new_tokens ** length_penalty``), or at ``max_new_tokens``, where the live beams finish;
        at most ``num_beams`` hypotheses are kept, the best ones.  ONE beam is greedy decoding and ends where ``generate`` ends: at the
        first EOS (the rule above would let the runner-up token live on past it), whatever ``length_penalty`` says.
        Returns the best hypothesis (``num_return > 1``: the list of the best ``num_return``), the last token dropped as ``generate``
        drops it.  ``update_cache=False``: the cache is sliced back.  ``update_cache=True``: the cache keeps the query and the best
        answer and ``prefill_ids`` grows as in ``generate`` - a hypothesis that was live at ``max_new_tokens`` has its rows in its
        parent's tail and is committed from there (``ForkedCache.commit``); one that ended in EOS earlier may have lost its slot to
        another beam, so its answer tokens run through the base cache in one sequential forward pass instead.  Sampling knobs are not
        used; ``num_beams=1`` gives ``generate``'s greedy tokens.  ``last_beam_hypotheses`` keeps ``(score, tokens)`` of the kept
        hypotheses of the last search, best first, every generated token included: the answers drop their last token, so the return
        value cannot say what a score was taken over.  A cache that cannot be forked is refused before a row is appended to it."""
        self._fork_limit("generate_beam", int(num_beams))
        B = int(num_beams)
        if not 1 <= int(num_return) <= B:
            raise ValueError(f"generate_beam: num_return={num_return} outside [1, num_beams={B}]")
        ForkedCache.check_base(kv, B)           # (the query's rows go to the base BEFORE the fork: ask now what fork() will ask)
        seen_prev = kv._seen_tokens
        input_ids = self._ids(query)
        max_new = self.gen_kwargs["max_new_tokens"]
        eos = set(self.eos_token_ids)
        lp = float(length_penalty)
        logp = torch.log_softmax(self.model(input_ids, past_key_values=kv, use_cache=True).logits[:, -1].float(), dim=-1)
        V = logp.shape[-1]
        pos0 = kv.get_seq_length()              # position of the first generated token
        fork = None
        live = [(0, [], 0.0)]                   # (row of logp = branch slot, generated tokens, summed log-probability)
        finished = []                           # (score, tokens, slot whose tail holds the rows of tokens[:-1] or None)
        n_gen = 0
        while live:
            rows = torch.tensor([h[0] for h in live], device=self.device)
            sums = torch.tensor([h[2] for h in live], dtype=torch.float32, device=self.device)
            cand = (logp[rows] + sums[:, None]).view(-1)
            top = torch.topk(cand, min(2 * B, cand.numel()))
            n_gen += 1
            nxt = []
            for rank, (val, idx) in enumerate(zip(top.values.tolist(), top.indices.tolist())):
                h, tok = live[idx // V], idx % V
                if tok in eos:
                    if rank < B:
                        finished.append((val / n_gen ** lp, h[1] + [tok], None))
                    continue
                nxt.append((h[0], h[1] + [tok], val))
                if len(nxt) == B:
                    break
            if B == 1 and finished:             # one beam: the greedy token is EOS, generate() stops here
                break
            if n_gen >= max_new:                # the token budget: the live beams finish, their rows still in their parents' tails
                finished += [(val / n_gen ** lp, toks, slot if fork is not None else None) for slot, toks, val in nxt]
                break
            finished = sorted(finished, key=lambda f: -f[0])[:B]
            if not nxt:
                break
            if len(finished) >= B:
                best_live = max(val for _, _, val in nxt)
                bound = best_live / (max_new if lp > 0 else n_gen) ** lp
                if bound <= finished[-1][0]:
                    break
            if fork is None:
                fork = kv.fork(B, tail_capacity=max(max_new, 1))
            slots = fork.reorder([p for p, _, _ in nxt])
            live = [(s, toks, val) for s, (_, toks, val) in zip(slots, nxt)]
            cur = torch.zeros((B, 1), dtype=torch.long, device=self.device)
            for s, toks, _ in live:
                cur[s] = toks[-1]
            pos = torch.full((B, 1), pos0 + n_gen - 1, dtype=torch.long, device=self.device)
            logp = torch.log_softmax(self.model(cur, past_key_values=fork, use_cache=True, position_ids=pos).logits[:, -1].float(), dim=-1)
        finished = sorted(finished, key=lambda f: -f[0])[:B]
        best = finished[0]
        self.last_beam_hypotheses = [(score, toks) for score, toks, _ in finished]   # best first; every token, the dropped last one included
        answers = [torch.tensor([toks[:-1]], dtype=torch.long, device=self.device).view(1, -1) for _, toks, _ in finished[:int(num_return)]]
        if update_cache and best[2] is not None:
            fork.commit(best[2])
        elif update_cache and answers[0].shape[1]:
            self.model.model(answers[0], past_key_values=kv, use_cache=True)
        self._end_turn(kv, update_cache, seen_prev, input_ids, answers[0])
        out = answers if return_ids else [self.decode(a) for a in answers]
        return out[0] if int(num_return) == 1 else out

    @_on_model_device
    @torch.inference_mode()
    def generate_samples(self, query: Union[str, torch.Tensor], kv, n: int, return_ids: bool = False) -> list:
        """``n`` answers to ONE query over one pruned cache (self-consistency, best-of-n; no reference counterpart).  The query's first
        step runs once on the base cache, on the sequential path; the answers are the branches of ``kv.fork(n)``, which sees the
        query rows as shared: every branch draws its own first token from the same logits (``gen_kwargs``: with ``do_sample=False``
        all answers are ``generate``'s) and the branches decode together as in ``generate_batch``, the tails holding generated tokens
        only.  More answers than one launch takes (``64 // G`` branches, at most 16) run in waves over the same query rows.  ``kv`` is
        sliced back afterwards: it is left as it was; one that cannot be forked is refused before a row is appended to it."""
        n = int(n)
        if n < 1:
            raise ValueError(f"generate_samples: n={n}")
        seen_prev = kv._seen_tokens
        input_ids = self._ids(query)
        wave = self._fork_wave()
        ForkedCache.check_base(kv, min(wave, n))   # (the query's rows go to the base BEFORE the fork: ask now what fork() will ask)
        first = self.model(input_ids, past_key_values=kv, use_cache=True).logits[:, -1]
        pos0 = kv.get_seq_length()
        answers: list = []
        for w0 in range(0, n, wave):    # every branch draws its first token from the query's logits
            B = min(wave, n - w0)
            fork = kv.fork(B, tail_capacity=max(self.gen_kwargs["max_new_tokens"], 1))
            answers += self._decode_slots(fork, [first] * B, [pos0] * B)
        kv.slice(seen_prev)
        return answers if return_ids else [self.decode(a) for a in answers]

    @_on_model_device
    @torch.inference_mode()
    def generate_multi(self, queries, kvs, update_cache: bool = False, return_ids: bool = False) -> list:
        """Responses to one query PER CACHE, decoded together (no reference counterpart: batch is 1 there): ``queries[i]`` is
        answered over ``kvs[i]``, a pruned slack-layout ``EvictCache`` of its own - several users, each with an own compressed
        context.  The first steps (the query tokens) of all sequences of a wave run as ONE packed forward pass over their caches
        (``multi_packed_first``, the default; ``False``: one forward per cache at batch 1 through the path ``generate`` takes); then
        all live sequences decode in one batch, one token each per step, whose attention is one launch per layer over all the caches
        (``kvcache.CacheBatch``) and whose other layers read the model's weights once for the whole batch.  Same knobs as ``generate``
        (``gen_kwargs``; the last token of every answer is dropped as there); a sequence stops at EOS or ``max_new_tokens`` while the
        others go on.  Afterwards every cache is sliced back to its previous length unless ``update_cache=True`` (multi-turn:
        ``prefill_ids`` grows as in ``generate``), and is an ordinary ``EvictCache`` again either way.  More caches than one launch
        takes (16, or ``128 // Hkv``) run in waves.  Answers agree with ``generate`` up to the summation order of the attention (an
        argmax may tie); with ``do_sample=True`` the draws of the sequences interleave."""
        kvs = list(kvs)
        ids = [self._ids(q) for q in queries]
        if len(ids) != len(kvs):
            raise ValueError(f"generate_multi: {len(ids)} queries for {len(kvs)} caches (one query per cache)")
        wave = max(1, min(self.multi_max_caches, 16, 128 // self.config.num_key_value_heads))
        answers: list = []
        for w0 in range(0, len(ids), wave):
            answers += self._generate_multi_wave(ids[w0:w0 + wave], kvs[w0:w0 + wave], update_cache)
        return answers if return_ids else [self.decode(a) for a in answers]

    def _packs_first_steps_multi(self, lengths: List[int]) -> bool:
        """Whether a wave of queries of these lengths (one per cache) takes the packed first step.  Every wave of two or more does;
        a shape rule - should a measurement show a shape at which one pass per cache is faster - goes HERE
        (tools/multi_prefill_bench.py).  (An empty query has no last position to take a token from: it goes to the
        per-cache loop, which fails on it as it always did.)"""
        return bool(self.multi_packed_first) and len(lengths) >= 2 and all(n > 0 for n in lengths)

    def _generate_multi_wave(self, ids: List[torch.Tensor], kvs: list, update_cache: bool) -> List[torch.Tensor]:
        B = len(ids)
        if B == 1:   # (nothing to share: the sequential path)
            return [self.generate(ids[0], kv=kvs[0], update_cache=update_cache, return_ids=True)]
        batch = CacheBatch(kvs)
        seen_prev = [kv._seen_tokens for kv in kvs]
        if self._packs_first_steps_multi([x.shape[1] for x in ids]):   # every query at the positions behind its own cache
            first, pos = self._packed_first(batch, ids, [kv.get_seq_length() for kv in kvs])
        else:
            first, pos = [], []
            for b in range(B):  # first step of every sequence: its query on its own cache, at batch 1
                first.append(self.model(ids[b], past_key_values=kvs[b], use_cache=True).logits[:, -1].clone())
                pos.append(kvs[b].get_seq_length())       # (the caches have different lengths: explicit positions from here on)
        answers = self._decode_slots(batch, first, pos)
        for b, kv in enumerate(kvs):
            self._end_turn(kv, update_cache, seen_prev[b], ids[b], answers[b])
        return answers

    def head_score(self, kv) -> torch.Tensor:
        """Per-(layer, KV head) maximum score ``[L, Hkv]`` — what the reference saves with ``--save_head_score``
        (test.py:22-25: ``torch.stack(kv.score, dim=0).squeeze().amax(-1)``) for context-independent, head-level eviction."""
        from . import ops
        score = kv._stacked_score(kv.score)
        if not score.is_cuda:  # (host-side scores, e.g. loaded from a file: no kernel needed)
            return score.reshape(score.shape[0], score.shape[-2], score.shape[-1]).amax(-1)
        return ops.rowmax(score.reshape(score.shape[0], score.shape[-2], score.shape[-1]))

    def save_head_score(self, kv, data: str, idx: int, head_score_dir: Optional[str] = None) -> str:
        """Write the head scores of ``kv`` where ``load_score=True`` looks for them: ``<dir>/<name>-<data>-<idx>.pt`` holding
        a ``[L, Hkv]`` tensor in the model dtype (reference test.py:22-25).  Several files of one model are combined by
        ``load_head_score`` with an element-wise maximum."""
        d = head_score_dir or self.head_score_dir
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"{head_score_name(self.name)}-{data}-{idx}.pt")
        torch.save(self.head_score(kv).cpu(), path)
        return path

    def eval_ratios(self, kv, ratios, fn, level: str = "pair"):
        """Multi-ratio evaluation from ONE prefill (reference eval.py:30-36): for every ratio ``kv.prune(ratio, level)`` on a
        non-evicting cache (``kv_type="retain"``: the mask is re-applied at every attention call) and ``fn(kv)``.
        Returns ``[([ratio, round(real_ratio, 4), round(thres, 4)], fn(kv)), ...]`` — the record layout of eval.py:34."""
        assert isinstance(kv, RetainCache), "several ratios from one prefill need the non-evicting cache (kv_type='retain')"
        out = []
        for ratio in ratios:
            thres, ratio_true = kv.prune(ratio, level)
            out.append(([ratio, round(ratio_true, 4), round(thres, 4)], fn(kv)))
        return out

    def eval_ratios_evict(self, kv, ratios, fn, level: str = "pair"):
        """``eval_ratios`` on the cache that really evicts (no reference counterpart): ONE prefill, then for every ratio
        ``kv.prune(ratio, level)`` - the first call prunes, every later one tightens the pruned cache (``EvictCache.tighten``) -
        and ``fn(kv)`` on a cache that decodes at the reduced size.  A pruned cache cannot take evicted pairs back, so the
        ratios must not increase: ``ValueError`` otherwise, before the cache is touched.  Same record layout as ``eval_ratios``."""
        ratios = list(ratios)
        if any(b > a for a, b in zip(ratios, ratios[1:])):
            raise ValueError(f"eval_ratios_evict: the ratios must be non-increasing (got {ratios}): an evicting cache only shrinks")
        out = []
        for ratio in ratios:
            thres, ratio_true = kv.prune(ratio, level)
            out.append(([ratio, round(ratio_true, 4), round(thres, 4)], fn(kv)))
        return out

    @_on_model_device
    @torch.inference_mode()
    def _prob(self, input_ids: torch.Tensor, kv=None, device: str = "cuda") -> torch.Tensor:
        """Next-token probabilities (reference model/wrapper.py:286-306)."""
        kv = self._init_kv(kv=kv)
        output = self.__call__(input_ids.to(self.device), kv, update_cache=False, return_logits=True)
        probs = torch.softmax(output.logits[0].float(), dim=-1).squeeze()
        return probs.cpu() if device == "cpu" else probs
