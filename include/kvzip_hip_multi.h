/*
 * kvzip_hip_multi.h — C ABI for one decode step over SEVERAL independent pruned KV caches in one launch (gfx950).
 *
 * No reference counterpart: the reference decodes one query over one cache at a time (batch is hard-wired to 1).  Here B pruned
 * caches of the same model geometry (Hkv, G, D, dtype), each in the slack layout of kvz_compact_plan - every head segment followed by
 * free rows - and each in its OWN flat K and V buffers, take one new token each: the call appends the token's K,V row to every head
 * segment of every live cache and attends the cache's G query rows per head over that segment, new row included.  The ragged
 * flash-decoding scheme of kvz_varlen_attn_append with S = B*Hkv segments instead of Hkv: work items are cut from the SUM of all
 * segment lengths (in multiples of 128 keys; every segment of a live cache gets at least one), one split launch and one combine
 * launch whatever B is.  kvz_fork_attn_append is the call for B queries over ONE cache.
 *
 * Same conventions as kvzip_hip.h: raw DEVICE pointers plus sizes, the HIP stream last, no allocation, no device synchronisation,
 * no host-to-device copy (the segment table travels as kernel arguments), 0 on success or a negative KVZ_E* code with the message in
 * kvz_last_error().  Arguments are validated on the host before any launch.  Arrays named *_host (and the two pointer tables) are
 * HOST arrays, read during the call only.
 */
#ifndef KVZIP_HIP_MULTI_H
#define KVZIP_HIP_MULTI_H

#include "kvzip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace of kvz_multi_attn_append (partial results of the key ranges; needs no initialisation).  Does not depend on
 * the key lengths; 0 for B <= 0 (or any other non-positive size). */
size_t kvz_multi_attn_workspace_bytes(int B, int Hkv, int G, int D);

/* One decode step of B caches.  For every cache b with offset_host[b] >= 0 and every head h, with
 *   row = seg_start_host[b*Hkv + h] + len_host[b*Hkv + h] + offset_host[b]:
 *   k_ptrs_host[b][row, :] = k_new[b, h, 0, :]   (same for v)      - the ONLY rows written, 2 * Hkv per live cache
 *   out[b, h, g, :] = softmax(scale * q[b, h, g, :] . K^T) V  over rows seg_start .. row of that segment (no mask: one query position)
 * offset_host[b] counts the rows appended to cache b BEFORE this call and must be below slack_host[b], the free rows behind every
 * segment of cache b (KVZ_EINVAL otherwise: the new row would land in the next segment).  offset_host[b] = -1 marks an inactive cache:
 * nothing of it is read or written, it gets no work item and its rows of `out` are zero.
 *   q                    [B, Hkv, G, D] contiguous
 *   k_ptrs_host, v_ptrs_host   HOST arrays of B DEVICE pointers: the flat [rows, D] K / V buffer of every cache
 *   seg_start_host, len_host   HOST int32 [B, Hkv]: first row and base length (rows kept by the prune) of every head segment
 *   k_new, v_new         [B, Hkv, 1, D], rows contiguous; batch and head strides in elements, multiples of 8
 *   out                  [B, Hkv, G, D] contiguous
 * Final normalisation out = fp16/bf16(a / l), as the decode combine of kvz_varlen_attn.
 * Limits: D in {64, 128}, B <= 16, Hkv <= 64, B*Hkv <= 128, G <= 64 (KVZ_EUNSUPPORTED otherwise). */
int kvz_multi_attn_append(const void* q, void* const* k_ptrs_host, void* const* v_ptrs_host, const int32_t* seg_start_host,
                          const int32_t* len_host, const int32_t* slack_host, const int32_t* offset_host, const void* k_new,
                          const void* v_new, int64_t k_new_batch_stride, int64_t k_new_head_stride, int64_t v_new_batch_stride,
                          int64_t v_new_head_stride, int B, int Hkv, int G, int D, float scale, int dtype, void* out, void* ws,
                          size_t ws_bytes, kvz_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KVZIP_HIP_MULTI_H */
