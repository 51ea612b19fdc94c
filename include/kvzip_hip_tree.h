/*
 * kvzip_hip_tree.h — C ABI for TREE speculative decoding on a pruned KV cache (gfx950): verify a tree of drafted tokens in one step,
 * then keep the rows of the accepted root-to-leaf path.
 *
 * No reference counterpart: the reference decodes one token per forward pass.  The verify step of kvzip_hip_spec.h feeds a CHAIN
 * through the model: the last accepted token and one proposed continuation.  Here the t new positions are the NODES of a tree in
 * topological order - node 0 is the last accepted token, every other node continues one earlier node - so several continuations
 * share one forward pass and one read of the kept rows.  Two things differ from the chain call:
 *   - the mask among the new rows: node p comes with a 64-bit ancestor mask, bit j set iff new row j is visible to node p
 *     (its ancestors and itself).  The old rows of a head segment stay visible to every node, unmasked;
 *   - the accepted path is not a prefix of the t appended rows: kvz_tree_keep_path moves row path[i] to slot i in every layer,
 *     in place, after which taking back the t - n rows behind the path is host bookkeeping as in the chain form.
 * Everything else is the chain call's: the slack layout of kvz_compact_plan, the workspace, the work-item cut, two launches per
 * layer whatever t is, new keys read from k_new / v_new and never from the rows the call writes.
 *
 * Same conventions as kvzip_hip.h: raw DEVICE pointers plus sizes, the HIP stream last, no allocation, no device synchronisation,
 * no host-to-device copy (masks, paths and tables travel as kernel arguments), 0 on success or a negative KVZ_E* code with the
 * message in kvz_last_error().  Arguments are validated on the host before any launch.
 */
#ifndef KVZIP_HIP_TREE_H
#define KVZIP_HIP_TREE_H

#include "kvzip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace of kvz_tree_attn_append: the size the chain verify call of kvzip_hip_spec.h needs for the same arguments
 * (needs no initialisation); 0 for t <= 0 (or any other non-positive size). */
size_t kvz_tree_attn_workspace_bytes(int t, int Hkv, int G, int D);

/* One verify step over a tree of t nodes.  Head h holds old = k_len[h] + k_len_offset rows from row k_start[h] on before the call.
 * For every node p < t:
 *   k_cache[k_start[h] + old + p, :] = k_new[h, p, :]   (same for v)      - the ONLY rows written, 2 * t per head, in node order
 *   out[h, p, g, :] = softmax(scale * q[h, p, g, :] . K^T) V   over the old rows (no mask) and the new rows j with bit j of
 *                     anc_host[p] set
 *   anc_host         HOST uint64 [t] (read during the call only, passed on by value): bit p of anc_host[p] is set (a node sees
 *                    itself), no bit above p (topological order), no bit at or above t
 * All other arguments, shapes, strides and the final normalisation out = fp16/bf16(a / l) are those of the chain verify call of
 * kvzip_hip_spec.h; with anc_host[p] = bits 0 .. p the result is bit-identical to that call's.
 * KVZ_EINVAL: as the chain call (a null or non-16-byte-aligned pointer, both metadata forms missing, a stride that is no multiple of
 *   8, t < 1, k_len_offset < 0, k_len_offset + t > slack, a negative segment start or length in k_meta_host, a bad dtype), and a
 *   null anc_host, a mask without its own bit, with a bit above its node or with a bit at or above t (the message names the node).
 * KVZ_EUNSUPPORTED: D not in {64, 128}, Hkv > 64, t*G > 64 query rows per KV head.
 * KVZ_EWORKSPACE: ws_bytes below kvz_tree_attn_workspace_bytes(t, Hkv, G, D). */
int kvz_tree_attn_append(const void* q, void* k_cache, void* v_cache, const int32_t* k_start, const int32_t* k_len, int k_len_offset,
                         const int32_t* k_meta_host, int slack, const void* k_new, const void* v_new, int64_t k_new_head_stride,
                         int64_t k_new_pos_stride, int64_t v_new_head_stride, int64_t v_new_pos_stride, int t, int Hkv, int G, int D,
                         float scale, int dtype, void* out, void* ws, size_t ws_bytes, const uint64_t* anc_host, kvz_stream_t stream);

/* Keep the accepted path of the t node rows a verify step appended, all layers in one launch (one further launch per table-full of
 * layers: the tables travel as kernel arguments).  For every layer l, head h and i < n:
 *   k_host[l][row0_host[l*Hkv + h] + i, :] = k_host[l][row0_host[l*Hkv + h] + path_host[i], :]      (same for v)
 * as if all rows were read before any is written (the move is in place: one entry's source slot may be another's destination).
 * Only the slots i with path_host[i] != i are written; an identity path launches nothing.
 *   k_host, v_host   HOST arrays [n_layers] of DEVICE pointers: the flat caches [rows, D] of the layers
 *   row0_host        HOST int32 [n_layers * Hkv]: the row of node 0's slot of (layer, head)
 *   path_host        HOST int32 [n], strictly ascending, path_host[i] >= i, path_host[n - 1] < t
 * KVZ_EINVAL: a null pointer (path_host may be null when n == 0), a null or non-16-byte-aligned cache pointer, n_layers, Hkv or D
 *   not positive, n < 0, t < 0, t > 64, a path that is not strictly ascending, path_host[i] < i, path_host[n - 1] >= t, a negative
 *   row0, a bad dtype.
 * KVZ_EUNSUPPORTED: a row of D elements that is no multiple of 16 bytes or longer than 1024 bytes, Hkv > 64. */
int kvz_tree_keep_path(int n_layers, void* const* k_host, void* const* v_host, const int32_t* row0_host, const int32_t* path_host, int n,
                       int t, int Hkv, int D, int dtype, kvz_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KVZIP_HIP_TREE_H */
