/*
 * kvzip_hip_spec.h — C ABI for one VERIFY step of draft-and-verify (speculative) decoding on a pruned KV cache (gfx950).
 *
 * No reference counterpart: the reference decodes one token per forward pass.  A verify step feeds t consecutive new positions of ONE
 * sequence - the last accepted token and t - 1 drafted ones - through the model in one pass.  On a pruned cache in the slack layout of
 * kvz_compact_plan (every head segment followed by free rows) the attention of such a pass is this call: it appends the t new K,V rows
 * behind every head segment and attends the t*G query rows of every KV head over the rows the segment held before, unmasked, plus the
 * new rows up to and including the row's own position.  The rows of the segments are read from memory once for up to 32 query rows
 * per KV head and twice for up to 64, whatever t is (the scheme of kvz_fork_attn_append with positions in the place of branches); the
 * t x t triangle over the new rows is a block of its own per head that takes the new keys from k_new / v_new, never from the rows the
 * call writes.  Two launches whatever t is.  Taking rejected positions back is host bookkeeping (a smaller k_len_offset at the next
 * call): their rows stay in the slack as garbage and are overwritten by the next step.
 *
 * Same conventions as kvzip_hip.h: raw DEVICE pointers plus sizes, the HIP stream last, no allocation, no device synchronisation,
 * no host-to-device copy (k_meta_host travels as kernel arguments), 0 on success or a negative KVZ_E* code with the message in
 * kvz_last_error().  Arguments are validated on the host before any launch.
 */
#ifndef KVZIP_HIP_SPEC_H
#define KVZIP_HIP_SPEC_H

#include "kvzip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace of kvz_spec_attn_append (partial results of the key ranges and of the triangle; needs no initialisation).
 * Does not depend on the key lengths; 0 for t <= 0 (or any other non-positive size). */
size_t kvz_spec_attn_workspace_bytes(int t, int Hkv, int G, int D);

/* One verify step.  Head h holds old = k_len[h] + k_len_offset rows from row k_start[h] on before the call.  For every position p < t:
 *   k_cache[k_start[h] + old + p, :] = k_new[h, p, :]   (same for v)      - the ONLY rows written, 2 * t per head
 *   out[h, p, g, :] = softmax(scale * q[h, p, g, :] . K^T) V   over the old rows (no mask) and the new rows 0 .. p
 *   q                [Hkv, t, G, D] contiguous (query row p*G + g of head h)
 *   k_cache, v_cache [rows, D] flat, slack layout
 *   k_start, k_len   DEVICE int32 [Hkv], and / or
 *   k_meta_host      HOST int32 [2*Hkv] = starts ++ lengths, passed on by value (read during the call only); when both forms are
 *                    given the kernels use k_meta_host
 *   k_len_offset     rows appended to every head BEFORE this call (>= 0); there is no device-side part of it
 *   slack            free rows behind every segment as the cache was laid out: k_len_offset + t must not exceed it (KVZ_EINVAL
 *                    otherwise: the new rows would land in the next segment)
 *   k_new, v_new     [Hkv, t, D], rows contiguous; head and position strides in elements, multiples of 8
 *   out              [Hkv, t, G, D] contiguous
 * Softmax in fp32 in the exp2 domain; final normalisation out = fp16/bf16(a / l), as the decode combine of kvz_varlen_attn.
 * KVZ_EINVAL: a null or non-16-byte-aligned pointer, both metadata forms missing, a stride that is no multiple of 8, t < 1,
 *   k_len_offset < 0, k_len_offset + t > slack, a negative segment start or length in k_meta_host, a bad dtype.
 * KVZ_EUNSUPPORTED: D not in {64, 128}, Hkv > 64, t*G > 64 query rows per KV head.
 * KVZ_EWORKSPACE: ws_bytes below kvz_spec_attn_workspace_bytes(t, Hkv, G, D). */
int kvz_spec_attn_append(const void* q, void* k_cache, void* v_cache, const int32_t* k_start, const int32_t* k_len, int k_len_offset,
                         const int32_t* k_meta_host, int slack, const void* k_new, const void* v_new, int64_t k_new_head_stride,
                         int64_t k_new_pos_stride, int64_t v_new_head_stride, int64_t v_new_pos_stride, int t, int Hkv, int G, int D,
                         float scale, int dtype, void* out, void* ws, size_t ws_bytes, kvz_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KVZIP_HIP_SPEC_H */
