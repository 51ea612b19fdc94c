/*
 * kvzip_hip_tighten.h — C ABI for tightening an already pruned KV cache to a smaller ratio (gfx950).
 *
 * No reference counterpart: the reference's EvictCache prunes once; several ratios from one prefill are only
 * offered by its RetainCache (eval.py:30-36), which never evicts.  Here a cache pruned with the mask `old` is
 * pruned again with a mask `new` that is a SUBSET of `old` (a smaller ratio over the same scores: all three
 * selection levels give nested masks).  Every row `new` keeps is still in the flat cache, so the dense K,V are
 * not needed: the gather reads the ragged layout of the old plan and writes the ragged layout of the new one.
 *
 * Same conventions as kvzip_hip.h: raw DEVICE pointers plus sizes, the HIP stream last, no allocation, no device
 * synchronisation, 0 on success or a negative KVZ_E* code with the message in kvz_last_error().  Arguments are
 * validated on the host before any launch.  Masks are one byte per context token ([layers*Hkv, N], tok1 = 1) or
 * ONE byte per (layer, head) row (head-level eviction, tok1 = 0), each mask with its own flag.  The new plan
 * (new_len_k, new_seg_start, new_tile_base, cu_len_k, max_len_k) comes from kvz_compact_plan /
 * kvz_compact_plan_heads on the new mask: there is no plan entry point of its own.
 */
#ifndef KVZIP_HIP_TIGHTEN_H
#define KVZIP_HIP_TIGHTEN_H

#include "kvzip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Number of positions of [rows, N] that new_valid keeps although old_valid evicted them, written to the int32
 * `count` (zeroed by the call on `stream`; one atomic add per block that found any).  Non-zero: the request would
 * have to bring evicted rows back, which no gather can do. */
int kvz_mask_resurrects(const uint8_t* new_valid, int new_tok1, const uint8_t* old_valid, int old_tok1,
                        int64_t rows, int N, int32_t* count /* zeroed by the call */, kvz_stream_t stream);

/* Gather of all layers in ONE launch from the ragged layout of the old plan into the ragged layout of the new one,
 * out of place (the outputs must not overlap the inputs):
 *   k_out[l][new_seg_start[r] + j, :] = k[l][old_seg_start[r] + (old rank of p_j), :]      (same for v)
 * for the j-th position p_j of row r = l*Hkv + h that BOTH full masks keep (full mask = ones(sink) ++ valid ++
 * ones(klen - sink - N), as in kvz_compact_plan); a position only the new mask keeps has no row to come from and is
 * skipped (kvz_mask_resurrects tells).  Rows appended after the old prune travel too: for i < tail_rows[l] row
 * old_seg_start[r] + old_len_k[r] + i  goes to  new_seg_start[r] + new_len_k[r] + i  (tail_rows[l] must not
 * exceed the slack of either layout).
 *   k_ptrs, v_ptrs         DEVICE arrays of `layers` pointers to the flat [rows, D] buffers of the old layout
 *   old_* / new_*          mask, tile_base [layers*Hkv, ntiles], seg_start and len_k [layers*Hkv] of each plan
 *                          (klen, sink, N and KVZ_COMPACT_TILE are those of both plans)
 *   tail_rows              device int32 [layers], or NULL = none
 *   k_out_ptrs, v_out_ptrs DEVICE arrays of `layers` pointers to the flat buffers of the new layout
 * D*elem_bytes must be a power of two in [64, 1024] (KVZ_EINVAL otherwise); rows are 16-byte aligned. */
int kvz_recompact_layers(const void* const* k_ptrs, const void* const* v_ptrs,          /* flat [rows, D] per layer */
                         const uint8_t* old_valid, int old_tok1, const int32_t* old_tile_base,
                         const int32_t* old_seg_start, const int32_t* old_len_k,
                         const uint8_t* new_valid, int new_tok1, const int32_t* new_tile_base,
                         const int32_t* new_seg_start, const int32_t* new_len_k,
                         const int32_t* tail_rows,                                        /* [layers] or NULL = none */
                         int layers, int Hkv, int N, int sink, int klen, int D, int elem_bytes,
                         void* const* k_out_ptrs, void* const* v_out_ptrs, kvz_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KVZIP_HIP_TIGHTEN_H */
