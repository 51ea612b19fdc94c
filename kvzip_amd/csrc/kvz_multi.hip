// kvz_multi.hip — one decode step (one new token each) over B INDEPENDENT pruned caches in one launch, gfx950.
//
// No reference counterpart: the reference decodes one query over one cache (batch is hard-wired to 1).  Several users,
// each with an own compressed context, generating at the same time pay B x (split + combine) launches per layer with kvz_varlen_attn_append -
// and the rest of the model reads all its weights once per user.  Here the B caches (same Hkv, G, D, dtype; slack layout; every cache
// in its OWN flat K and V buffers) are S = B*Hkv ragged segments of ONE launch:
//   multi_attn_split_kernel    the ragged flash-decoding scheme of varlen_attn_split2_kernel<APPEND> (kvz_attn.hip): work items are cut
//                              from the SUM of all S segment lengths in multiples of 128 keys (a 128 k-token cache beside a 4 k-token one
//                              gets 32 x the blocks), every segment of a live cache gets at least one item (an empty segment - a dropped
//                              head of a head-level cache - still receives its new row and attends to it alone).  The block that owns a
//                              segment's last key range first writes the segment's new K and V row into the slack of cache b (16-byte
//                              vector stores, workgroup barrier) and reads it back like any other key; no other block touches that row
//                              (G > 16: the row tiles of that range each write the same bytes and read behind their own barrier).
//                              S^T = K.Q^T on v_mfma_f32_16x16x32 with K rows straight from HBM, V through the padded per-wave LDS tile
//                              and ds_read_b64_tr_b16, fp32 softmax state in registers - the tile scheme of kvz_attn.hip unchanged.
//   multi_attn_combine_kernel  per (segment, group row): merges the partials of the segment's key ranges, out = fp16/bf16(a / l) (the
//                              'div' form of tests/attn_probes.py); rows of an inactive cache (offset -1) are zero.
// The combine stays a second launch: merging inside the split kernel needs a device-scope counter and a fence whose serial tail costs more
// than the launch (round 2, see the header of kvz_attn.hip); no block waits for another one.
// Segment table: the host knows every length, so the table - K,V base pointers and offsets per cache, start, base length and FIRST WORK ITEM
// per segment - travels BY VALUE as kernel arguments (2 KB of the 4 KB there are): no device table, no upload,
// nothing to keep in step with the caches.  A block finds its (segment, key range) with wave-uniform scalar work from those prefixes
// (up to 127 compares against constant kernel-argument offsets): batches of scalar loads from the kernel-argument segment, independent of
// each other.
#include "kvz_combine.h"
#include "../../include/kvzip_hip_multi.h"

#include <limits.h>

namespace kvz {
namespace multi {

constexpr int MK_THREADS = 512;
constexpr int MK_WAVES = 8;
constexpr int MK_MAXB = 16;          // caches
constexpr int MK_MAXH = 64;          // KV heads
constexpr int MK_MAXS = 128;         // segments: B * Hkv
constexpr int MK_MAXG = 64;          // query heads per KV head
constexpr int MK_SCAN = 16;          // prefix entries compared per batch of scalar loads

// the segment table, by value.  Segment s = b * Hkv + h.  Work items are numbered segment after segment: segment s owns items
// item0[s] .. item0[s + 1] - 1 (none when cache b is inactive).
struct Table {
    void* k[MK_MAXB];                      // flat [rows, D] buffers of cache b
    void* v[MK_MAXB];
    int32_t off[MK_MAXB];                  // rows appended before this step; -1: inactive
    int32_t start[MK_MAXS];                // first row of segment s
    int32_t len[MK_MAXS];                  // base length of segment s (the step sees len + off + 1 keys)
    int32_t item0[MK_MAXS + 1];            // first item of segment s; item0[S] = all items, INT_MAX behind (the scan reads in batches)
};

template <typename T, int D>
__global__ __launch_bounds__(MK_THREADS) void multi_attn_split_kernel(
    const T* __restrict__ q, Table tb, const T* __restrict__ k_new, const T* __restrict__ v_new, int64_t kn_bstride, int64_t kn_hstride,
    int64_t vn_bstride, int64_t vn_hstride, int S, int Hkv, int G, int chunk, float scale, float* __restrict__ part_o,
    float* __restrict__ part_ml, int n_rtiles) {
    typedef TileCfg<D> C;
    typedef typename Half<T>::v8 v8;
    // ---- this block's work item: (cache, head, key range) from the item prefixes (all wave-uniform scalar work) ----
    const int bx = blockIdx.x;             // (the grid has exactly as many blocks as there are items)
    int s = 0;             // the last segment whose first item is not beyond bx (segments without items share the next one's)
#pragma unroll
    for (int c = 0; c < MK_MAXS / MK_SCAN; ++c)
        if (c * MK_SCAN < S) {
#pragma unroll
            for (int j = c ? 0 : 1; j < MK_SCAN; ++j) s += bx >= tb.item0[c * MK_SCAN + j] ? 1 : 0;
        }
    const int b = s / Hkv;
    const int h = s - b * Hkv;
    const int rt = blockIdx.y;
    const int len = tb.len[s] + tb.off[b] + 1;      // the keys attended to include the token appended by this call
    const int64_t seg = tb.start[s];
    const int split = bx - tb.item0[s];
    const int c0 = split * chunk;
    const int c1 = min(len, c0 + chunk);
    // (plain pointers: the new row is written and read back by this block)
    const char* kbase = reinterpret_cast<const char*>(tb.k[b]) + seg * C::ROW_BYTES;
    const char* vbase = reinterpret_cast<const char*>(tb.v[b]) + seg * C::ROW_BYTES;
    if (c1 == len) {
        constexpr int CH = D * 2 / 16;  // 16-byte chunks per row
        if ((int)threadIdx.x < 2 * CH) {
            const bool is_v = (int)threadIdx.x >= CH;
            const int c = (int)threadIdx.x - (is_v ? CH : 0);
            const char* src = reinterpret_cast<const char*>(is_v ? v_new + b * vn_bstride + h * vn_hstride
                                                                 : k_new + b * kn_bstride + h * kn_hstride) + c * 16;
            char* dst = const_cast<char*>(is_v ? vbase : kbase) + (int64_t)(len - 1) * C::ROW_BYTES + c * 16;
            *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
        }
        __syncthreads();  // (workgroup-scope release/acquire: the row is visible to the loads of this block below)
    }
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int l15 = lane & 15, quad = lane >> 4;

    constexpr int BLOCK_WAVES = MK_WAVES;
    __shared__ __attribute__((aligned(16))) char lds[MK_WAVES * C::WAVE_LDS];
    char* wl = lds + wave * C::WAVE_LDS;

    const int n_qrows = G;
    const int64_t q_row0 = (int64_t)s * G;
#include "kvz_decode_state.inc"
    auto visible = [&](int key) -> bool { return qvalid && key < c1; };   // (one query position: every key of the segment is visible)

    auto load_tile = [&](u32x4 (&kr)[2][C::KK], u32x4 (&vr)[C::VLOADS], int t0) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            int key = t0 + sub * 16 + l15;
            key = key < len ? key : len - 1;  // clamp (masked below)
            const char* kp = kbase + (int64_t)key * C::ROW_BYTES + quad * 16;
#pragma unroll
            for (int kk = 0; kk < C::KK; ++kk) kr[sub][kk] = *reinterpret_cast<const u32x4*>(kp + kk * 64);
        }
#pragma unroll
        for (int it = 0; it < C::VLOADS; ++it) {
            const int c = it * WAVE + lane;
            int key = t0 + c / C::CPR;
            key = key < len ? key : len - 1;
            vr[it] = *reinterpret_cast<const u32x4*>(vbase + (int64_t)key * C::ROW_BYTES + (c % C::CPR) * 16);
        }
    };
#include "kvz_decode_step.inc"
#include "kvz_decode_loop.inc"

    const int64_t pbase = ((int64_t)bx * n_rtiles + rt) * TILE_RT;  // partial slot of this item
#include "kvz_decode_merge.inc"
}

// merge, per (segment, group row), the partials of the segment's key ranges.  grid = (S, G); the body is combine_partials of
// kvz_combine.h.  Rows of an inactive cache are zero.
template <typename T, int D>
__global__ __launch_bounds__(CB_THREADS) void multi_attn_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                                       Table tb, int Hkv, int G, int n_rtiles, T* __restrict__ out) {
    const int s = blockIdx.x, g = blockIdx.y;
    const int tid = threadIdx.x;
    const int64_t orow = ((int64_t)s * G + g) * D;
    if (tb.off[s / Hkv] < 0) {  // inactive cache
        if (tid < D) out[orow + tid] = (T)0.f;
        return;
    }
    const int first_item = tb.item0[s];
    const int n = tb.item0[s + 1] - first_item;   // (>= 1: every segment of a live cache has an item)
    const int64_t base = ((int64_t)first_item * n_rtiles + g / TILE_RT) * TILE_RT + g % TILE_RT;
    const int64_t istride = (int64_t)n_rtiles * TILE_RT;
    combine_partials<T, D>(n, [&](int s2) -> Partial {
        const int64_t pi = base + s2 * istride;
        return Partial{part_ml + pi * 2, part_o + pi * D};
    }, out + orow);
}

struct MultiWs { float* part_ml; float* part_o; size_t items; size_t bytes; };
static inline MultiWs multi_ws(void* ws, int B, int Hkv, int G, int D) {
    const int S = B * Hkv, n_rtiles = (G + TILE_RT - 1) / TILE_RT;
    MultiWs w;
    w.items = (size_t)target_items(S) + S;
    char* p = reinterpret_cast<char*>(ws);
    w.part_ml = reinterpret_cast<float*>(p);
    p += align256(w.items * n_rtiles * TILE_RT * 2 * sizeof(float));
    w.part_o = reinterpret_cast<float*>(p);
    p += align256(w.items * n_rtiles * TILE_RT * D * sizeof(float));
    w.bytes = (size_t)(p - reinterpret_cast<char*>(ws));
    return w;
}

template <typename T, int D>
static int launch_multi(const void* q, const Table& tb, int items, int chunk, const void* k_new, const void* v_new, int64_t kn_b,
                        int64_t kn_h, int64_t vn_b, int64_t vn_h, int B, int Hkv, int G, float scale, void* out, const MultiWs& w,
                        hipStream_t stream) {
    const int n_rtiles = (G + TILE_RT - 1) / TILE_RT;
    ProfScope ps("multi_attn", stream);
    if (items > 0) {  // (no live cache: nothing to attend, the combine writes the zeros)
        hipLaunchKernelGGL((multi_attn_split_kernel<T, D>), dim3(items, n_rtiles), dim3(MK_THREADS), 0, stream,
                           reinterpret_cast<const T*>(q), tb, reinterpret_cast<const T*>(k_new), reinterpret_cast<const T*>(v_new), kn_b,
                           kn_h, vn_b, vn_h, B * Hkv, Hkv, G, chunk, scale, w.part_o, w.part_ml, n_rtiles);
        KVZ_CHECK_LAUNCH("multi_attn_split_kernel");
    }
    hipLaunchKernelGGL((multi_attn_combine_kernel<T, D>), dim3(B * Hkv, G), dim3(CB_THREADS), 0, stream, w.part_o, w.part_ml, tb, Hkv, G,
                       n_rtiles, reinterpret_cast<T*>(out));
    KVZ_CHECK_LAUNCH("multi_attn_combine_kernel");
    return KVZ_OK;
}

}  // namespace multi
}  // namespace kvz

using namespace kvz;

extern "C" size_t kvz_multi_attn_workspace_bytes(int B, int Hkv, int G, int D) {
    if (B <= 0 || Hkv <= 0 || G <= 0 || D <= 0) return 0;
    return multi::multi_ws(nullptr, B, Hkv, G, D).bytes;
}

extern "C" int kvz_multi_attn_append(const void* q, void* const* k_ptrs_host, void* const* v_ptrs_host, const int32_t* seg_start_host,
                                     const int32_t* len_host, const int32_t* slack_host, const int32_t* offset_host, const void* k_new,
                                     const void* v_new, int64_t k_new_batch_stride, int64_t k_new_head_stride, int64_t v_new_batch_stride,
                                     int64_t v_new_head_stride, int B, int Hkv, int G, int D, float scale, int dtype, void* out, void* ws,
                                     size_t ws_bytes, kvz_stream_t stream_) {
    using namespace kvz::multi;
    hipStream_t stream = (hipStream_t)stream_;
    KVZ_REQUIRE(q && k_ptrs_host && v_ptrs_host && seg_start_host && len_host && slack_host && offset_host && k_new && v_new && out && ws,
                KVZ_EINVAL, "kvz_multi_attn_append: null pointer");
    KVZ_REQUIRE(B > 0 && Hkv > 0 && G > 0, KVZ_EINVAL, "kvz_multi_attn_append: bad shape (B %d, Hkv %d, G %d)", B, Hkv, G);
    KVZ_REQUIRE(D == 64 || D == 128, KVZ_EUNSUPPORTED, "kvz_multi_attn_append: head_dim %d unsupported (64 or 128)", D);
    KVZ_REQUIRE(B <= MK_MAXB && Hkv <= MK_MAXH && (int64_t)B * Hkv <= MK_MAXS && G <= MK_MAXG, KVZ_EUNSUPPORTED,
                "kvz_multi_attn_append: %d caches x %d KV heads x %d query heads per KV head unsupported (B <= %d, Hkv <= %d, "
                "B*Hkv <= %d segments, G <= %d)", B, Hkv, G, MK_MAXB, MK_MAXH, MK_MAXS, MK_MAXG);
    KVZ_REQUIRE(dtype == KVZ_F16 || dtype == KVZ_BF16, KVZ_EINVAL, "kvz_multi_attn_append: bad dtype %d", dtype);
    KVZ_REQUIRE(aligned16(q) && aligned16(k_new) && aligned16(v_new) && aligned16(out) && aligned16(ws), KVZ_EINVAL,
                "kvz_multi_attn_append: pointers must be 16-byte aligned");
    KVZ_REQUIRE(k_new_batch_stride % 8 == 0 && k_new_head_stride % 8 == 0 && v_new_batch_stride % 8 == 0 && v_new_head_stride % 8 == 0,
                KVZ_EINVAL, "kvz_multi_attn_append: the strides of the new rows must be multiples of 8 elements");
    const int S = B * Hkv;
    Table tb;
    int64_t total = 0;
    for (int b = 0; b < MK_MAXB; ++b) {
        tb.k[b] = tb.v[b] = nullptr;
        tb.off[b] = -1;
        if (b >= B) continue;
        const int off = offset_host[b];
        KVZ_REQUIRE(k_ptrs_host[b] && v_ptrs_host[b], KVZ_EINVAL, "kvz_multi_attn_append: null K or V pointer of cache %d", b);
        KVZ_REQUIRE(aligned16(k_ptrs_host[b]) && aligned16(v_ptrs_host[b]), KVZ_EINVAL,
                    "kvz_multi_attn_append: K and V of cache %d must be 16-byte aligned", b);
        KVZ_REQUIRE(off >= -1 && off < slack_host[b], KVZ_EINVAL,
                    "kvz_multi_attn_append: offset[%d] = %d outside [-1, slack = %d): the new row does not fit behind the segments", b, off,
                    slack_host[b]);
        tb.k[b] = k_ptrs_host[b];
        tb.v[b] = v_ptrs_host[b];
        tb.off[b] = off;
        for (int h = 0; h < Hkv; ++h) {
            const int s = b * Hkv + h;
            KVZ_REQUIRE(seg_start_host[s] >= 0 && len_host[s] >= 0 && (int64_t)seg_start_host[s] + len_host[s] + slack_host[b] <= INT_MAX,
                        KVZ_EINVAL, "kvz_multi_attn_append: bad segment start %d or length %d of cache %d, head %d", seg_start_host[s],
                        len_host[s], b, h);
            if (off >= 0) total += (int64_t)len_host[s] + off + 1;
        }
    }
    const MultiWs w = multi_ws(ws, B, Hkv, G, D);
    KVZ_REQUIRE(ws_bytes >= w.bytes, KVZ_EWORKSPACE, "kvz_multi_attn_append: workspace too small (%zu bytes, %zu needed)", ws_bytes, w.bytes);
    // the key ranges: chunks of the SUM of the live segment lengths, a multiple of 128 keys; every live segment at least one
    const int target = target_items(S);
    const int64_t chunk64 = chunk_of(total, target);
    KVZ_REQUIRE(chunk64 <= INT_MAX - 128, KVZ_EINVAL, "kvz_multi_attn_append: %lld keys in one step", (long long)total);
    const int chunk = (int)chunk64;
    int items = 0;
    for (int s = 0; s <= MK_MAXS; ++s) {
        tb.item0[s] = s <= S ? items : INT_MAX;
        if (s < MK_MAXS) { tb.start[s] = 0; tb.len[s] = 0; }
        if (s >= S) continue;
        const int b = s / Hkv;
        tb.start[s] = seg_start_host[s];
        tb.len[s] = len_host[s];
        if (tb.off[b] >= 0) {
            const int len = len_host[s] + tb.off[b] + 1;
            items += (len + chunk - 1) / chunk;     // (len >= 1)
        }
    }
    KVZ_REQUIRE((size_t)items <= w.items, KVZ_EWORKSPACE, "kvz_multi_attn_append: %d work items exceed the %zu the workspace holds", items,
                w.items);
#define KVZ_MULTI_ARGS q, tb, items, chunk, k_new, v_new, k_new_batch_stride, k_new_head_stride, v_new_batch_stride, v_new_head_stride, B, \
                       Hkv, G, scale, out, w, stream
#define KVZ_MULTI_CALL(T, DD) return launch_multi<T, DD>(KVZ_MULTI_ARGS)
    KVZ_DISPATCH_HALF_D(dtype, D, KVZ_MULTI_CALL);
#undef KVZ_MULTI_CALL
#undef KVZ_MULTI_ARGS
}
