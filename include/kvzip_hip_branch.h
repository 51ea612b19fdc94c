/*
 * kvzip_hip_branch.h — C ABI for moving branch-private rows between the branch slots of a forked decode (gfx950).
 *
 * No reference counterpart: the reference decodes one query over one cache (batch is hard-wired to 1).  The branches of a fork
 * (kvz_fork_attn_append, kvzip_hip_prefill.h) share the pruned cache read-only and each owns a private tail per layer,
 * [B, Hkv, tail_cap, D].  A beam search continues "beam b from beam p's state" at every step: the rows of p's tail have to be in
 * b's slot before the next decode step.  kvz_fork_branch_copy does that for all layers, all (src, dst) pairs, all heads, K and V in
 * ONE launch; the caller plans the pairs so that a surviving hypothesis stays where it is (kvcache.plan_branch_reorder: the number of
 * copies is the number of dropped hypotheses).
 *
 * Same conventions as kvzip_hip.h: raw DEVICE pointers plus sizes, the HIP stream last, no allocation, no device synchronisation,
 * no host-to-device copy (the pointer and capacity tables and the pair list travel as kernel arguments), 0 on success or a negative
 * KVZ_E* code with the message in kvz_last_error().  Arguments are validated on the host before any launch.  Arrays named *_host are
 * HOST arrays, read during the call only.
 */
#ifndef KVZIP_HIP_BRANCH_H
#define KVZIP_HIP_BRANCH_H

#include "kvzip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For every layer l < n_layers, pair i < n_pairs and head h < Hkv:
 *   tail_k_host[l][dst_host[i], h, 0 : rows_host[i], :] = tail_k_host[l][src_host[i], h, 0 : rows_host[i], :]   (same for v)
 * - the ONLY bytes written: rows >= rows_host[i] of a destination, the sources and every other slot keep what they hold.
 *   tail_k_host, tail_v_host   HOST arrays of n_layers DEVICE pointers: the [B, Hkv, tail_cap_host[l], D] contiguous tails of layer l
 *   tail_cap_host              HOST int32 [n_layers]: rows per (slot, head) of layer l (the capacities may differ between layers)
 *   src_host, dst_host, rows_host   HOST int32 [n_pairs]
 * Hazard-free by contract: the set of source slots and the set of destination slots are disjoint and no destination appears twice
 * (one source may feed several destinations), so the copy runs in place with no ordering between blocks and no second buffer.
 * KVZ_EINVAL: a null or non-16-byte-aligned pointer, a slot outside [0, B), src == dst, a slot on both sides, a repeated destination,
 *   rows_host[i] < 0 or rows_host[i] > tail_cap_host[l] for any layer, a non-positive size.
 * KVZ_EUNSUPPORTED: D * elem_size not a multiple of 16, B > 16, Hkv > 64.
 * n_pairs == 0 (src_host, dst_host, rows_host may then be null) or all rows_host[i] == 0: a successful no-op, nothing is launched.
 * One launch carries up to 128 layers (their pointers and capacities are 2.5 KB of the 4 KB of kernel arguments, the pairs another
 * 192 bytes); a model with more layers gets one further launch per 128 layers, issued by this call on the same stream. */
int kvz_fork_branch_copy(void* const* tail_k_host, void* const* tail_v_host, const int32_t* tail_cap_host, int n_layers,
                         int B, int Hkv, int D, int elem_size,
                         const int32_t* src_host, const int32_t* dst_host, const int32_t* rows_host, int n_pairs,
                         kvz_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KVZIP_HIP_BRANCH_H */
