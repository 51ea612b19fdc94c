// kvz_tree.hip — tree speculative decoding on a pruned slack-layout cache (gfx950): verify a TREE of t drafted nodes in one step, then
// keep the node rows of the accepted path.  No reference counterpart: the reference decodes one token per forward pass.
//
// tree_attn_kernel       the first launch of a verify step (kvz_spec.hip) with ONE difference: the t new positions are the nodes of a
//                        tree in topological order, and the triangle item tests bit j of the ancestor mask of the query row's node
//                        instead of j <= p.  Everything else is spec_block of kvz_spec_step.h: the shared items, the workspace, the
//                        work-item cut, the row copy by the triangle block of tile group 0, new keys from k_new / v_new only.  The
//                        masks travel by value (t <= 64: 512 bytes of kernel arguments).  c1 of a triangle block stays "last
//                        position of the tile group + 1": nodes are in topological order, nothing above the diagonal is visible.
//                        The second launch is spec_combine_kernel of kvz_spec.hip, unchanged (every node sees itself).
// tree_keep_path_kernel  after a tree verify step the slack of every (layer, head) holds the t node rows in node order.  The accepted root-to-leaf path is an ascending
// list path[0 .. n) with path[i] >= i; row path[i] has to be at slot i, K and V, before the next step.  The rows behind slot n - 1
// are then taken back on the host like the rejected tail of a chain.
//   grid.x  (head, K or V)
//   grid.y  layer
// A block owns the t slots of one (layer, head, K or V): nobody else touches them, so the move is in place.  One entry's source slot
// can be another's destination ([1, 2, 3]: slot 1 is read for slot 0 and written from slot 2), so a block loads EVERY row that moves
// into registers (16-byte loads, at most 64 rows of at most 1024 bytes: 16 vectors per lane), passes a workgroup barrier, and only
// then stores.  Entries with path[i] == i are not in the move list: their rows are not written.
// Tables: the host knows every address, so the per-layer pointers, the row of node 0 per (layer, head) and the move list travel BY
// VALUE as kernel arguments (the method of kvz_fork_branch.hip) - no device table, no upload.  A launch takes KP_MAXL layers and
// KP_MAXROW0 (layer, head) pairs; models beyond that take one further launch per table-full.
#include "kvz_spec_step.h"
#include "../../include/kvzip_hip_spec.h"
#include "../../include/kvzip_hip_tree.h"

namespace kvz {
namespace spec {

template <typename T, int D, int NT>
__global__ __launch_bounds__(SP_THREADS) void tree_attn_kernel(
    const T* __restrict__ q, T* k, T* v, const int32_t* __restrict__ k_start, const int32_t* __restrict__ k_len, int k_len_offset,
    HeadMeta hm, int host_meta, const T* __restrict__ k_new, const T* __restrict__ v_new, int64_t kn_hstride, int64_t kn_pstride,
    int64_t vn_hstride, int64_t vn_pstride, int t, int Hkv, int G, int target_items, float scale, float* __restrict__ part_o,
    float* __restrict__ part_ml, int n_rtiles, AncMasks anc) {
#define KVZ_SPEC_TREE true
#define KVZ_SPEC_ANC (&anc)
#include "kvz_spec_block.inc"
#undef KVZ_SPEC_TREE
#undef KVZ_SPEC_ANC
}

template <typename T, int D>
static int launch_tree(const void* q, void* k, void* v, const int32_t* k_start, const int32_t* k_len, int k_len_offset,
                       const int32_t* meta_host, const void* k_new, const void* v_new, int64_t kn_h, int64_t kn_p, int64_t vn_h,
                       int64_t vn_p, int t, int Hkv, int G, float scale, int dtype, void* out, void* ws, const AncMasks& anc,
                       hipStream_t stream) {
    const SpecPlan p = spec_plan(meta_host, t, Hkv, G, D, ws);
    ProfScope ps("tree_attn", stream);
#define KVZ_TREE_LAUNCH(NT)                                                                                                              \
    hipLaunchKernelGGL((tree_attn_kernel<T, D, NT>), p.grid, dim3(SP_THREADS), 0, stream, reinterpret_cast<const T*>(q),                \
                       reinterpret_cast<T*>(k), reinterpret_cast<T*>(v), k_start, k_len, k_len_offset, p.hm, p.host,                    \
                       reinterpret_cast<const T*>(k_new), reinterpret_cast<const T*>(v_new), kn_h, kn_p, vn_h, vn_p, t, Hkv, G,         \
                       p.target, scale, p.w.part_o, p.w.part_ml, p.n_rtiles, anc)
    if (p.nt == 2) KVZ_TREE_LAUNCH(2);
    else KVZ_TREE_LAUNCH(1);
#undef KVZ_TREE_LAUNCH
    KVZ_CHECK_LAUNCH("tree_attn_kernel");
    return spec_combine(p, k_len, k_len_offset, t, Hkv, G, D, dtype, out, stream);
}

}  // namespace spec

namespace tree {

constexpr int KP_THREADS = 256;
constexpr int KP_MAXT = 64;           // node rows of a step (one bit each in the masks of the verify call)
constexpr int KP_MAXL = 64;           // layers of one launch
constexpr int KP_MAXROW0 = 640;       // (layer, head) pairs of one launch
constexpr int KP_MAXH = 64;           // KV heads
constexpr int KP_MAXROWBYTES = 1024;
constexpr int KP_VECS = KP_MAXT * (KP_MAXROWBYTES / 16) / KP_THREADS;   // 16-byte vectors per lane at the largest move

struct Table {
    void* k[KP_MAXL];                 // flat cache [rows, D] of layer l
    void* v[KP_MAXL];
    int32_t row0[KP_MAXROW0];         // [l * Hkv + h]: the row of node 0's slot
    uint8_t src[KP_MAXT];             // the entries that move: slot src[i] -> slot dst[i], dst[i] < src[i]
    uint8_t dst[KP_MAXT];
};
static_assert(sizeof(Table) + 64 <= 4096, "the tables travel as kernel arguments");

__global__ __launch_bounds__(KP_THREADS) void tree_keep_path_kernel(Table tb, int n_moves, int Hkv, int row_bytes) {
    const int layer = blockIdx.y;
    const int h = blockIdx.x >> 1;
    const int is_v = blockIdx.x & 1;
    const int vpr = row_bytes >> 4;                                          // 16-byte vectors per row
    const int n16 = n_moves * vpr;                                           // <= KP_VECS * KP_THREADS (host-checked)
    char* base = reinterpret_cast<char*>(is_v ? tb.v[layer] : tb.k[layer]) + (int64_t)tb.row0[layer * Hkv + h] * row_bytes;
    u32x4 r[KP_VECS];
    int to[KP_VECS];                                                         // byte offset of the destination
#pragma unroll
    for (int u = 0; u < KP_VECS; ++u) {
        const int e = u * KP_THREADS + threadIdx.x;
        if (e < n16) {
            const int mv = e / vpr, c = e - mv * vpr;
            r[u] = *reinterpret_cast<const u32x4*>(base + (int)tb.src[mv] * row_bytes + c * 16);
            to[u] = (int)tb.dst[mv] * row_bytes + c * 16;
        }
    }
    __syncthreads();   // every row that moves is in registers: from here on its slot may be overwritten
#pragma unroll
    for (int u = 0; u < KP_VECS; ++u) {
        const int e = u * KP_THREADS + threadIdx.x;
        if (e < n16) *reinterpret_cast<u32x4*>(base + to[u]) = r[u];
    }
}

}  // namespace tree
}  // namespace kvz

using namespace kvz;

extern "C" size_t kvz_tree_attn_workspace_bytes(int t, int Hkv, int G, int D) { return kvz_spec_attn_workspace_bytes(t, Hkv, G, D); }

extern "C" int kvz_tree_attn_append(const void* q, void* k_cache, void* v_cache, const int32_t* k_start, const int32_t* k_len,
                                    int k_len_offset, const int32_t* k_meta_host, int slack, const void* k_new, const void* v_new,
                                    int64_t k_new_head_stride, int64_t k_new_pos_stride, int64_t v_new_head_stride,
                                    int64_t v_new_pos_stride, int t, int Hkv, int G, int D, float scale, int dtype, void* out, void* ws,
                                    size_t ws_bytes, const uint64_t* anc_host, kvz_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* who = "kvz_tree_attn_append";
    KVZ_REQUIRE(anc_host, KVZ_EINVAL, "%s: null pointer", who);
    const int rc = spec::spec_validate(who, q, k_cache, v_cache, k_start, k_len, k_len_offset, k_meta_host, slack, k_new, v_new,
                                       k_new_head_stride, k_new_pos_stride, v_new_head_stride, v_new_pos_stride, t, Hkv, G, D, dtype, out,
                                       ws);
    if (rc != KVZ_OK) return rc;
    // (1 <= t <= 64 from here on; a shift by 64 is undefined, so the bits at or above t, or above 63, are named without one)
    spec::AncMasks anc;
    const uint64_t beyond = t >= 64 ? 0 : ~uint64_t(0) << t;
    for (int p = 0; p < spec::SP_MAXROWS; ++p) anc.m[p] = 0;
    for (int p = 0; p < t; ++p) {
        const uint64_t m = anc_host[p];
        const uint64_t above = p >= 63 ? 0 : ~uint64_t(0) << (p + 1);
        KVZ_REQUIRE((m >> p) & 1, KVZ_EINVAL, "%s: the mask of node %d lacks bit %d (a node sees itself)", who, p, p);
        KVZ_REQUIRE(!(m & beyond), KVZ_EINVAL, "%s: the mask of node %d has a bit at or above t = %d", who, p, t);
        KVZ_REQUIRE(!(m & above), KVZ_EINVAL, "%s: the mask of node %d has a bit above %d (nodes come in topological order)", who, p, p);
        anc.m[p] = m;
    }
    KVZ_REQUIRE(ws_bytes >= kvz_tree_attn_workspace_bytes(t, Hkv, G, D), KVZ_EWORKSPACE, "%s: workspace too small (%zu bytes, %zu needed)",
                who, ws_bytes, kvz_tree_attn_workspace_bytes(t, Hkv, G, D));
#define KVZ_TREE_ARGS q, k_cache, v_cache, k_start, k_len, k_len_offset, k_meta_host, k_new, v_new, k_new_head_stride, k_new_pos_stride, \
                      v_new_head_stride, v_new_pos_stride, t, Hkv, G, scale, dtype, out, ws, anc, stream
#define KVZ_TREE_CALL(T, DD) return spec::launch_tree<T, DD>(KVZ_TREE_ARGS)
    KVZ_DISPATCH_HALF_D(dtype, D, KVZ_TREE_CALL);
#undef KVZ_TREE_CALL
#undef KVZ_TREE_ARGS
}

extern "C" int kvz_tree_keep_path(int n_layers, void* const* k_host, void* const* v_host, const int32_t* row0_host,
                                  const int32_t* path_host, int n, int t, int Hkv, int D, int dtype, kvz_stream_t stream_) {
    using namespace kvz::tree;
    hipStream_t stream = (hipStream_t)stream_;
    KVZ_REQUIRE(k_host && v_host && row0_host, KVZ_EINVAL, "kvz_tree_keep_path: null pointer");
    KVZ_REQUIRE(n >= 0, KVZ_EINVAL, "kvz_tree_keep_path: n = %d path entries", n);
    KVZ_REQUIRE(n == 0 || path_host, KVZ_EINVAL, "kvz_tree_keep_path: null pointer");
    KVZ_REQUIRE(n_layers > 0 && Hkv > 0 && D > 0, KVZ_EINVAL, "kvz_tree_keep_path: bad shape (layers %d, Hkv %d, D %d)", n_layers, Hkv, D);
    KVZ_REQUIRE(t >= 0 && t <= KP_MAXT, KVZ_EINVAL, "kvz_tree_keep_path: t = %d node rows (0 .. %d)", t, KP_MAXT);
    KVZ_REQUIRE(dtype == KVZ_F16 || dtype == KVZ_BF16, KVZ_EINVAL, "kvz_tree_keep_path: bad dtype %d", dtype);
    const int64_t rb64 = (int64_t)D * 2;
    KVZ_REQUIRE(rb64 % 16 == 0 && rb64 <= KP_MAXROWBYTES, KVZ_EUNSUPPORTED,
                "kvz_tree_keep_path: D * elem_size = %lld bytes per row unsupported (a multiple of 16, at most %d)", (long long)rb64,
                KP_MAXROWBYTES);
    KVZ_REQUIRE(Hkv <= KP_MAXH, KVZ_EUNSUPPORTED, "kvz_tree_keep_path: %d KV heads unsupported (Hkv <= %d)", Hkv, KP_MAXH);
    for (int i = 0; i < n; ++i) {
        KVZ_REQUIRE(path_host[i] >= i, KVZ_EINVAL, "kvz_tree_keep_path: path[%d] = %d is below %d (slot i takes a row from slot i or later)", i,
                    path_host[i], i);
        KVZ_REQUIRE(i == 0 || path_host[i] > path_host[i - 1], KVZ_EINVAL,
                    "kvz_tree_keep_path: path[%d] = %d does not ascend from path[%d] = %d", i, path_host[i], i - 1, path_host[i - 1]);
    }
    KVZ_REQUIRE(n == 0 || path_host[n - 1] < t, KVZ_EINVAL, "kvz_tree_keep_path: path[%d] = %d names no node of the t = %d", n - 1,
                n ? path_host[n - 1] : 0, t);
    for (int l = 0; l < n_layers; ++l) {
        KVZ_REQUIRE(k_host[l] && v_host[l], KVZ_EINVAL, "kvz_tree_keep_path: null K or V cache of layer %d", l);
        KVZ_REQUIRE(aligned16(k_host[l]) && aligned16(v_host[l]), KVZ_EINVAL,
                    "kvz_tree_keep_path: the caches of layer %d must be 16-byte aligned", l);
        for (int h = 0; h < Hkv; ++h)
            KVZ_REQUIRE(row0_host[(int64_t)l * Hkv + h] >= 0, KVZ_EINVAL, "kvz_tree_keep_path: negative row0 of layer %d, head %d", l, h);
    }
    Table tb;
    int n_moves = 0;
    for (int i = 0; i < KP_MAXT; ++i) tb.src[i] = tb.dst[i] = 0;
    for (int i = 0; i < n; ++i)
        if (path_host[i] != i) {
            tb.src[n_moves] = (uint8_t)path_host[i];
            tb.dst[n_moves] = (uint8_t)i;
            ++n_moves;
        }
    if (n_moves == 0) return KVZ_OK;   // an identity path: nothing moves, nothing is launched
    const int row_bytes = (int)rb64;
    const int per = KP_MAXROW0 / Hkv < KP_MAXL ? KP_MAXROW0 / Hkv : KP_MAXL;   // layers of one launch
    ProfScope ps("tree_keep_path", stream);
    for (int l0 = 0; l0 < n_layers; l0 += per) {
        const int nl = n_layers - l0 < per ? n_layers - l0 : per;
        for (int l = 0; l < KP_MAXL; ++l) {
            tb.k[l] = l < nl ? k_host[l0 + l] : nullptr;
            tb.v[l] = l < nl ? v_host[l0 + l] : nullptr;
        }
        for (int i = 0; i < KP_MAXROW0; ++i) tb.row0[i] = i < nl * Hkv ? row0_host[(int64_t)l0 * Hkv + i] : 0;
        hipLaunchKernelGGL(tree_keep_path_kernel, dim3((unsigned)(Hkv * 2), (unsigned)nl), dim3(KP_THREADS), 0, stream, tb, n_moves, Hkv,
                           row_bytes);
        KVZ_CHECK_LAUNCH("tree_keep_path_kernel");
    }
    return KVZ_OK;
}
