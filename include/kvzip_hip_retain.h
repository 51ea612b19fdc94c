/*
 * kvzip_hip_retain.h — C ABI for attention over a DENSE KV cache through an index of kept rows (gfx950): the data path of RetainCache.
 *
 * Reference: RetainCache (attention/kvcache.py:216-347) keeps the full KV of the context and subsamples it with a boolean mask in front
 * of every attention call.  Here the mask becomes, once per prune, an index: for every (layer, KV head) the ascending list of the
 * positions of the dense [Hkv, capacity, D] store that the full mask ones(sink) ++ valid keeps.  Attention then reads the kept rows
 * where they lie - no copy, no plan and no host round trip per call - and computes what kvz_varlen_attn computes on the compacted copy
 * of the same rows, bit for bit: the same cut into work items over the sum of the head lengths, the same 32-key wave tile, the same
 * merge of a block's waves, the same combine.  Only the row addresses differ.
 *
 * Key j of head h, which has n_h indexed positions from entry start_h of the index on:
 *   j <  n_h :  pos = idx[start_h + j]
 *   j >= n_h :  pos = ctx_end + (j - n_h)          (ctx_end = sink + N: the rows behind the context - query and generated tokens - are
 *                                                   kept by every head, so they are computed, not stored)
 *   row address = store + (h * head_stride + pos * D) * 2 bytes
 * Head h sees n_h + fill - ctx_end keys (fill = rows in use per head), one more with the append form.  Positions are clamped to the rows
 * in use before they become addresses: a stale or foreign index gives wrong numbers, never an access outside the store.
 *
 * Same conventions as kvzip_hip.h: raw DEVICE pointers plus sizes, the HIP stream last, no allocation, no device synchronisation,
 * no host-to-device copy (the per-head metadata travels as kernel arguments), 0 on success or a negative KVZ_E* code with the message
 * in kvz_last_error().  Arguments are validated on the host before any launch.  No device-side offset: these calls are not meant for
 * graph capture.
 */
#ifndef KVZIP_HIP_RETAIN_H
#define KVZIP_HIP_RETAIN_H

#include "kvzip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Index of kept positions, all layers in ONE launch (a block per (layer, head, 1024-token tile), as the gather of kvz_compact_layers).
 *   valid       [layers, Hkv, N] bytes (kvz_retain_index) or one byte per (layer, head) (kvz_retain_index_heads: head-level masks)
 *   tile_base   [layers * Hkv, ceil((sink + N) / 1024)] as written by kvz_compact_plan / kvz_compact_plan_heads with klen = sink + N
 *               (slack is irrelevant): the kept rows of a head in front of each tile.  Lengths come from the same plan call (len_k).
 *   row_start   DEVICE int32 [layers * Hkv]: first entry of every (layer, head) in idx - the caller packs the rows back to back
 *               (exclusive prefix of the plan's len_k)
 *   idx         int32 [idx_len]: entry row_start[r] + i = the i-th kept position (ascending, in [0, sink + N)) of row r.  The ONLY
 *               memory written; an entry that would fall at or behind idx_len is not written.
 * KVZ_EINVAL: null pointer, idx or row_start not 4-byte aligned, layers / Hkv <= 0, layers * Hkv > 65535, N < 0, sink < 0,
 *   sink + N <= 0, idx_len < 0. */
int kvz_retain_index(const uint8_t* valid, int layers, int Hkv, int N, int sink, const int32_t* tile_base, const int32_t* row_start,
                     int32_t* idx, int64_t idx_len, kvz_stream_t stream);
int kvz_retain_index_heads(const uint8_t* valid_heads, int layers, int Hkv, int N, int sink, const int32_t* tile_base,
                           const int32_t* row_start, int32_t* idx, int64_t idx_len, kvz_stream_t stream);

/* Bytes of the workspace of the two attention calls (partial results of the key ranges; needs no initialisation): the size
 * kvz_varlen_attn_workspace_bytes gives for the same (Hkv, G, q_len, D).  0 for a non-positive size or a row count q_len * G the
 * calls do not take. */
size_t kvz_retain_attn_workspace_bytes(int Hkv, int G, int q_len, int D);

/* Attention of q_len >= 1 new positions whose K, V rows are in the store already (rows fill - q_len .. fill - 1).
 *   q                [Hkv, q_len, G, D] contiguous (query row p*G + g of head h)
 *   k_store, v_store [Hkv, capacity, D]: rows contiguous, head stride head_stride elements (a multiple of 8, >= capacity * D)
 *   idx, idx_len     the index (all layers) and its length in entries, at least 1
 *   meta_host        HOST int32 [2 * Hkv] = start_h ++ n_h of this layer's heads, passed on by value (read during the call only)
 *   ctx_end, fill    sink + N and the rows in use per head; fill >= ctx_end + q_len
 *   causal           bottom-right aligned: position p sees the keys up to len_h - q_len + p
 *   out              [Hkv, q_len, G, D] contiguous = what kvz_varlen_attn returns on the compacted copy
 * KVZ_EINVAL: null or non-16-byte-aligned pointer (idx: 4 bytes), head_stride no multiple of 8 or below capacity * D, fill > capacity,
 *   fill < ctx_end + q_len, ctx_end < 0, idx_len < 1, a negative start or count, a count above ctx_end, start + count > idx_len, bad
 *   dtype, Hkv / G / q_len <= 0.
 * KVZ_EUNSUPPORTED: D not in {64, 128}, Hkv > 64, q_len * G above the row count at which kvz_varlen_attn hands over to kvz_flash_fwd.
 * KVZ_EWORKSPACE: ws_bytes below kvz_retain_attn_workspace_bytes(Hkv, G, q_len, D). */
int kvz_retain_attn(const void* q, const void* k_store, const void* v_store, int64_t head_stride, int capacity, const int32_t* idx,
                    int64_t idx_len, const int32_t* meta_host, int ctx_end, int fill, int Hkv, int G, int q_len, int D, float scale,
                    int causal, int dtype, void* out, void* ws, size_t ws_bytes, kvz_stream_t stream);

/* Decode step (q_len = 1) in one call: writes the new token's K, V into row `fill` of every head of the store - the ONLY rows written,
 * by the block that owns the last key range of the head, 16 bytes per store - and attends q over n_h + fill - ctx_end + 1 keys.  Equals
 * kvz_dense_append followed by kvz_retain_attn with fill + 1.
 *   q            [Hkv, G, D] contiguous;  out likewise
 *   k_new, v_new [Hkv, 1, D]: rows contiguous, head strides in elements (multiples of 8)
 * Errors as kvz_retain_attn with: fill >= ctx_end, fill + 1 <= capacity. */
int kvz_retain_attn_append(const void* q, void* k_store, void* v_store, int64_t head_stride, int capacity, const void* k_new,
                           const void* v_new, int64_t k_new_head_stride, int64_t v_new_head_stride, const int32_t* idx,
                           int64_t idx_len, const int32_t* meta_host, int ctx_end, int fill, int Hkv, int G, int D, float scale,
                           int dtype, void* out, void* ws, size_t ws_bytes, kvz_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KVZIP_HIP_RETAIN_H */
