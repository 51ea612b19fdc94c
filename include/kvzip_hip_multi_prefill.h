/*
 * kvzip_hip_multi_prefill.h — C ABI for the PACKED first step over SEVERAL independent pruned KV caches (gfx950): the query tokens of
 * B users, each with a pruned cache of its own, in ONE pass.
 *
 * No reference counterpart: the reference processes one query over one cache at a time (batch is hard-wired to 1).
 * kvz_multi_attn_append decodes one token for B independent caches in one launch; the caches' FIRST steps (their query tokens,
 * q_len > 1) ran one cache at a time.  Here the queries of the B caches lie back to back in one packed sequence of T = cu_q[B]
 * positions, and one call appends every cache's new K,V rows to the slack behind its head segments and attends every packed position
 * over its OWN cache's segment plus its own run's rows up to itself: a varlen-batched prefill over S = B*Hkv ragged segments.  One
 * split launch and one combine launch whatever B and T are.  kvz_fork_prefill_tail is the call for B queries over ONE shared cache.
 *
 * Same conventions as kvzip_hip.h: raw DEVICE pointers plus sizes, the HIP stream last, no allocation, no device synchronisation,
 * no host-to-device copy (the tables travel as kernel arguments), 0 on success or a negative KVZ_E* code with the message in
 * kvz_last_error().  Arguments are validated on the host before any launch.  Arrays named *_host (and the two pointer tables) are
 * HOST arrays, read during the call only.
 */
#ifndef KVZIP_HIP_MULTI_PREFILL_H
#define KVZIP_HIP_MULTI_PREFILL_H

#include "kvzip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace of kvz_multi_prefill for T packed positions of B caches: the fp32 partial results (m, l, a[D]) of the work
 * items, 64 query rows each.  With RG = Hkv * (T*G / 64 + B), an upper bound of the groups of 64 query rows of all segments, and
 * `target` the attn_items knob (default: the compute units of the device minus B*Hkv, a quarter of them from 3/4 of them on):
 *   items = target + 2 * RG             (key ranges: at most target + RG; one item per group for the run's own rows: RG)
 *   bytes = align256(items * 64 * 2 * 4) + align256(items * 64 * D * 4)
 * Worst case per packed position: Hkv * G / 32 items of 64 * (D + 2) * 4 bytes, i.e. Hkv * G * (D + 2) * 8 bytes (29 KB for
 * Hkv 4, G 7, D 128), on top of (target + 2 * B * Hkv) items.  Depends on (T, B, Hkv, G, D) only, never on the key lengths; needs no
 * initialisation.  0 for T <= 0 (or any other non-positive size). */
size_t kvz_multi_prefill_workspace_bytes(int T, int B, int Hkv, int G, int D);

/* Cache b owns the packed positions cu_q_host[b] .. cu_q_host[b+1] - 1 (n_b of them).  cu_q_host[0] = 0, the array is non-decreasing,
 * T = cu_q_host[B].  With old = len_host[b*Hkv + h] + offset_host[b] and row0 = seg_start_host[b*Hkv + h], for packed position i of
 * cache b, p = i - cu_q_host[b], head h, group member g:
 *   keys(i)         = K_b[row0 : row0 + old] ++ k_new[h, cu_q[b] : cu_q[b] + p + 1]      (values alike; bottom-right causal inside the
 *                     run; nothing of another cache is ever visible)
 *   out[h, i, g, :] = fp16/bf16(a / l), a and l the fp32 numerator and denominator of softmax(scale * q . keys^T) V, merged over all
 *                     partial results in the exp2 domain: ONE fp32 division and ONE cast (the 'div' form of kvz_multi_attn_append)
 *   K_b[row0 + old + j, :] = k_new[h, cu_q[b] + j, :]  for j < n_b  (V alike)  - the ONLY rows written, 2 * Hkv * n_b per
 *                     participating cache
 * n_b = 0: the cache takes no part - nothing of it is read or written, offset_host[b] (and its pointers) are ignored.
 * offset_host[b] + n_b > slack_host[b] -> KVZ_EINVAL (the rows would run into the next segment); offset_host[b] < 0 with n_b > 0 ->
 * KVZ_EINVAL.  An empty segment (old = 0: a dropped head of a head-level cache) attends its new rows alone.
 *   q                    element (h, g, i, d) at q[h*q_stride_head + g*q_stride_group + i*q_stride_pos + d]; strides in elements,
 *                        multiples of 8 (as kvz_flash_fwd takes them)
 *   cu_q_host            HOST int32 [B + 1]
 *   k_ptrs_host, v_ptrs_host   HOST arrays of B DEVICE pointers: the flat [rows, D] K / V buffer of every cache
 *   seg_start_host, len_host   HOST int32 [B, Hkv]: first row and base length (rows kept by the prune) of every head segment
 *   slack_host           HOST int32 [B]: free rows behind every segment of cache b
 *   offset_host          HOST int32 [B]: rows appended to cache b BEFORE this call
 *   k_new, v_new         [Hkv, T, D] through head and position strides in elements (multiples of 8), rows contiguous
 *   out                  [Hkv, T, G, D] contiguous
 *   ws, ws_bytes         kvz_multi_prefill_workspace_bytes(T, B, Hkv, G, D) bytes at least (KVZ_EWORKSPACE otherwise)
 * Keys at or beyond `old` are read from k_new / v_new, never from the slack rows written by this call, so no block waits for another
 * block's write.  T = 0 is a successful no-op.  Limits: D in {64, 128}, B <= 16, Hkv <= 64, B*Hkv <= 128, G <= 64 (KVZ_EUNSUPPORTED
 * otherwise); null or misaligned pointers, bad strides, bad dtype and bad cu_q -> KVZ_EINVAL. */
int kvz_multi_prefill(const void* q, int64_t q_stride_head, int64_t q_stride_group, int64_t q_stride_pos, const int32_t* cu_q_host,
                      void* const* k_ptrs_host, void* const* v_ptrs_host, const int32_t* seg_start_host, const int32_t* len_host,
                      const int32_t* slack_host, const int32_t* offset_host, const void* k_new, const void* v_new,
                      int64_t k_new_head_stride, int64_t k_new_pos_stride, int64_t v_new_head_stride, int64_t v_new_pos_stride, int B,
                      int Hkv, int G, int D, float scale, int dtype, void* out, void* ws, size_t ws_bytes, kvz_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KVZIP_HIP_MULTI_PREFILL_H */
