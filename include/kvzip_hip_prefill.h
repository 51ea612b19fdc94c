/*
 * kvzip_hip_prefill.h — C ABI for the PACKED first step of a forked decode (gfx950): the query tokens of several branches of one
 * shared pruned KV cache in ONE pass.
 *
 * No reference counterpart: the reference processes one query at a time (batch is hard-wired to 1).  kvz_fork_attn_append decodes one
 * token of B branches in one launch; the branches' FIRST steps (their query tokens, q_len > 1) ran one branch at a time.  Here the
 * queries of B branches lie back to back in one packed sequence of T = cu_q[B] positions.  The attention over the shared segments
 * has no mask (the whole context precedes every query), so kvz_flash_fwd (causal = 0, with its LSE) takes all T positions as they
 * are; kvz_fork_prefill_tail then does everything that is private to a branch in one launch: it appends the branch's new K,V rows
 * to its tail, attends every packed position over its OWN branch's tail (bottom-right causal; rows of other branches are never
 * visible) and merges that with the shared partial result by the two LSEs.
 *
 * Same conventions as kvzip_hip.h: raw DEVICE pointers plus sizes, the HIP stream last, no allocation, no device synchronisation,
 * no host-to-device copy (the tables travel as kernel arguments), 0 on success or a negative KVZ_E* code with the message in
 * kvz_last_error().  Arguments are validated on the host before any launch.  Arrays named *_host are HOST arrays, read during the call
 * only.
 */
#ifndef KVZIP_HIP_PREFILL_H
#define KVZIP_HIP_PREFILL_H

#include "kvzip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace of kvz_fork_prefill_tail for T packed positions of B branches.  0: a block walks the whole tail of its query
 * rows, so there are no partial results to keep (`ws` may then be NULL). */
size_t kvz_fork_prefill_workspace_bytes(int T, int B, int Hkv, int G, int D);

/* Branch b owns the packed positions cu_q_host[b] .. cu_q_host[b+1] - 1 (n_b of them; n_b = 0: the branch takes no part, nothing of it
 * is read or written).  branch_host = NULL: b is also the branch's index in the tails.  Otherwise branch_host is a HOST int32 [B]
 * permutation of 0 .. B-1 and the b-th run of positions belongs to tail branch_host[b] - a packing that does not name the branches in
 * ascending order; `tail`, t_b and tail_len_host below are then those of branch_host[b].
 * With t_b = tail_len_host[b], for packed position i of branch b, p = i - cu_q_host[b], head h, group member g:
 *   keys(i)          = tail[b, h, 0 : t_b] ++ k_new[h, cu_q_host[b] : cu_q_host[b] + p + 1]        (values alike)
 *   o_tail, lse_tail = softmax(scale * q[h, g, i, :] . keys^T) V  in fp32
 *   out[h, i, g, :]  = merge of (o_shared[h, i, g, :], lse_shared[h, i, g]) and (o_tail, lse_tail) as kvz_attn_merge_lse merges
 *                      (weights exp(lse - max lse), normalised by their sum), cast ONCE to the 16-bit type
 *   tail[b, h, t_b : t_b + n_b, :] = k_new / v_new[h, cu_q_host[b] : cu_q_host[b+1], :]            - the ONLY tail rows written
 *   q                    element (h, g, i, d) at q[h*q_stride_head + g*q_stride_group + i*q_stride_pos + d]; strides in elements,
 *                        multiples of 8 (as kvz_flash_fwd takes them)
 *   cu_q_host            HOST int32 [B + 1], cu_q_host[0] = 0, non-decreasing; T = cu_q_host[B]
 *   tail_k, tail_v       [B, Hkv, tail_cap, D] contiguous
 *   tail_len_host        HOST int32 [B]: rows in use before the call (>= 0; t_b + n_b <= tail_cap)
 *   k_new, v_new         [Hkv, T, D] through head and position strides in elements (multiples of 8), rows contiguous
 *   o_shared             [Hkv, T, G, D] contiguous, 16-bit; lse_shared [Hkv, T, G] fp32, natural log of the scaled logits, -inf: that
 *                        side saw no key (its row of o_shared is then ignored whatever it holds) - what kvz_flash_fwd writes with
 *                        o strides (T*G*D, D, G*D)
 *   out                  [Hkv, T, G, D] contiguous; may be o_shared itself
 * Keys at or beyond t_b are read from k_new / v_new, never from the tail, so no block waits for another block's write.
 * T = 0 is a successful no-op.  Limits: D in {64, 128}, B <= 16, Hkv <= 64, G <= 64 (KVZ_EUNSUPPORTED otherwise). */
int kvz_fork_prefill_tail(const void* q, int64_t q_stride_head, int64_t q_stride_group, int64_t q_stride_pos, const int32_t* cu_q_host,
                          void* tail_k, void* tail_v, int tail_cap, const int32_t* tail_len_host, const void* k_new, const void* v_new,
                          int64_t k_new_head_stride, int64_t k_new_pos_stride, int64_t v_new_head_stride, int64_t v_new_pos_stride,
                          const void* o_shared, const float* lse_shared, void* out, const int32_t* branch_host, int B, int Hkv, int G,
                          int D, float scale, int dtype, void* ws, size_t ws_bytes, kvz_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KVZIP_HIP_PREFILL_H */
