// kvz_retain.hip — attention over a DENSE KV cache through an index of kept rows (gfx950): the data path of RetainCache.
//
// Reference: RetainCache (attention/kvcache.py:216-347) applies its boolean mask in front of every attention call (boolean indexing,
// a fresh flat copy of every kept row per layer and token).  Here:
//   retain_index_kernel    once per prune, all layers in one launch: a block per (layer, head, 1024-token tile) - the geometry of
//                          compact_gather_kernel - turns the mask into the ascending list of kept positions.  The kept rows in front of a
//                          tile come from the plan (tile_base of kvz_compact_plan with klen = sink + N); only the index is written.
//   retain_attn_kernel     the split-key decode scheme of varlen_attn_split2_kernel (kvz_attn.hip) with the row address of a key taken
//                          from the index: the same cut into work items over the SUM of the head lengths, the same 32-key wave tile, the same
//                          merge of the 8 waves.  The arithmetic - expressions and their order - is that of kvz_attn.hip, so the result
//                          is the bits of kvz_varlen_attn on the compacted copy.
//   retain_combine_kernel  combine_partials of kvz_combine.h over the head's key ranges, on by-value metadata.
// Q fragment, tile step and merge are the text that kernel includes too (kvz_decode_*.inc); the key loop is this
// file's own, since it also looks ahead in the index.
//
// Positions.  A lane holds the position of ONE key of a tile (key t0 + (lane & 31)); the K and V loads take theirs through a lane
// shuffle, so a tile costs one 4-byte index load per lane instead of one in front of each of its 2 + VLOADS row loads.  The index load
// is a dependent load in front of the row loads: the positions of tile t + 2*T_STEP are requested before the rows of tile t + T_STEP,
// whose positions were requested one iteration earlier and have arrived since.  Like the row loads they are issued unconditionally
// (clamped keys), so the loop has no load under a branch (see the comment of kvz_decode_loop.inc).
#include "kvz_combine.h"
#include "../../include/kvzip_hip_retain.h"

namespace kvz {
namespace retain {

// ---- index ---------------------------------------------------------------------------------------------------------------------
constexpr int CT = KVZ_COMPACT_TILE;  // tokens per tile
constexpr int IX_THREADS = 256;
constexpr int IX_PER_THREAD = CT / IX_THREADS;
static_assert(IX_PER_THREAD == 4, "tile/threads layout (full_mask4)");

__global__ __launch_bounds__(IX_THREADS) void retain_index_kernel(const uint8_t* __restrict__ valid, int tok1, int Hkv, int N, int sink,
                                                                 int ntiles, const int32_t* __restrict__ tile_base,
                                                                 const int32_t* __restrict__ row_start, int32_t* __restrict__ idx,
                                                                 int64_t idx_len) {
    const int tile = blockIdx.x;
    const int row = blockIdx.z * Hkv + blockIdx.y;
    const int klen = sink + N;
    __shared__ int wtot[IX_THREADS / WAVE];

    const uint8_t* vrow = valid + (int64_t)row * (tok1 ? N : 1);
    const int p0 = tile * CT + threadIdx.x * IX_PER_THREAD;
    const uint32_t bits = full_mask4(vrow, p0, sink, N, klen, tok1);
    const int c = __popc(bits);
    const int inc = wave_inclusive_scan(c);
    if (lane_id() == 63) wtot[threadIdx.x >> 6] = inc;
    __syncthreads();
    int pre = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) pre += wtot[w];
    int64_t o = (int64_t)row_start[row] + tile_base[(int64_t)row * ntiles + tile] + pre + inc - c;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (bits & (1u << j)) {
            if (o >= 0 && o < idx_len) idx[o] = p0 + j;
            ++o;
        }
}

// ---- attention -----------------------------------------------------------------------------------------------------------------
constexpr int RT_THREADS = 512;
constexpr int RT_WAVES = 8;
constexpr int RT_MAXH = 64;
struct HeadMeta { int32_t start[RT_MAXH]; int32_t cnt[RT_MAXH]; };

// `tail` = keys behind the indexed ones (fill - ctx_end, + 1 with APPEND); `rows` = rows of a head that may be read (fill, + 1 with APPEND)
template <typename T, int D, bool APPEND>
__global__ __launch_bounds__(RT_THREADS) void retain_attn_kernel(
    const T* __restrict__ q, const T* k, const T* v, int64_t head_stride, const int32_t* __restrict__ idx, int64_t idx_len, HeadMeta hm,
    int ctx_end, int tail, int rows, int Hkv, int G, int q_len, int target_items, float scale, int causal, float* part_o, float* part_ml,
    int n_rtiles, const T* __restrict__ k_new, const T* __restrict__ v_new, int64_t kn_head_stride, int64_t vn_head_stride) {
    typedef TileCfg<D> C;
    typedef typename Half<T>::v8 v8;
    auto len_of = [&](int hh) -> int { return hm.cnt[hh] + tail; };
    // ---- this block's work item: (head, key range) from the ragged lengths (all wave-uniform scalar work) ----
    int total = 0;
    for (int hh = 0; hh < Hkv; ++hh) total += len_of(hh);
    const int chunk = chunk_of(total, target_items);
    int h = -1, split = 0, first_item = 0;
    {
        int b = blockIdx.x, items = 0;
        for (int hh = 0; hh < Hkv; ++hh) {
            const int n = max(1, (len_of(hh) + chunk - 1) / chunk);  // (an empty head still gets one item: it writes zeros)
            if (h < 0) {
                if (b < n) { h = hh; split = b; first_item = items; }
                else b -= n;
            }
            items += n;
        }
    }
    if (h < 0) return;  // beyond the last item
    const int rt = blockIdx.y;
    const int len = len_of(h);
    const int n_idx = hm.cnt[h];
    const int64_t istart = hm.start[h];
    const int c0 = split * chunk;
    const int c1 = min(len, c0 + chunk);
    const char* kbase = reinterpret_cast<const char*>(k + h * head_stride);
    const char* vbase = reinterpret_cast<const char*>(v + h * head_stride);
    if (APPEND && c1 == len) {
        // the new token's row: the last key of the head (position rows - 1), written by the one block that reads it
        constexpr int CH = D * 2 / 16;  // 16-byte chunks per row
        if ((int)threadIdx.x < 2 * CH) {
            const bool is_v = (int)threadIdx.x >= CH;
            const int c = (int)threadIdx.x - (is_v ? CH : 0);
            const char* src = reinterpret_cast<const char*>(is_v ? v_new + h * vn_head_stride : k_new + h * kn_head_stride) + c * 16;
            char* dst = const_cast<char*>(is_v ? vbase : kbase) + (int64_t)(rows - 1) * (D * 2) + c * 16;
            *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
        }
        __syncthreads();  // (workgroup-scope release/acquire: the row is visible to the loads of this block below)
    }
    const int R = q_len * G;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int l15 = lane & 15, quad = lane >> 4;

    constexpr int BLOCK_WAVES = RT_WAVES;
    __shared__ __attribute__((aligned(16))) char lds[RT_WAVES * C::WAVE_LDS];
    char* wl = lds + wave * C::WAVE_LDS;

    const int n_qrows = R;
    const int64_t q_row0 = (int64_t)h * R;
#include "kvz_decode_state.inc"
    int limit = causal ? (qrow / G) + len - q_len : len - 1;  // last visible key of this lane's query row (bottom-right aligned)
    if (!qvalid) limit = -1;
    auto visible = [&](int key) -> bool { return key <= limit && key < c1; };

    // the index entry of this lane's key of the tile at t0 (key t0 + (lane & 31), clamped like the row loads; an entry is read for the
    // computed keys as well - the last one of the head - so that the load is unconditional)
    const int lk = lane & 31;
    auto request_pos = [&](int t0) -> int {
        int key = t0 + lk;
        key = key < n_idx ? key : n_idx - 1;
        int64_t e = istart + (key > 0 ? key : 0);
        e = e < idx_len ? e : idx_len - 1;
        return idx[e];
    };
    // ... and the position it stands for, clamped to the rows in use (masked below where the key is beyond the range)
    auto position = [&](int entry, int t0) -> int {
        int key = t0 + lk;
        key = key < len ? key : len - 1;  // clamp (masked below)
        int pos = key < n_idx ? entry : ctx_end + (key - n_idx);
        pos = pos < rows ? pos : rows - 1;
        return pos > 0 ? pos : 0;
    };
    auto load_tile = [&](u32x4 (&kr)[2][C::KK], u32x4 (&vr)[C::VLOADS], int pos) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int p = __shfl(pos, sub * 16 + l15, 64);
            const char* kp = kbase + (int64_t)p * C::ROW_BYTES + quad * 16;
#pragma unroll
            for (int kk = 0; kk < C::KK; ++kk) kr[sub][kk] = *reinterpret_cast<const u32x4*>(kp + kk * 64);
        }
#pragma unroll
        for (int it = 0; it < C::VLOADS; ++it) {
            const int c = it * WAVE + lane;
            const int p = __shfl(pos, c / C::CPR, 64);
            vr[it] = *reinterpret_cast<const u32x4*>(vbase + (int64_t)p * C::ROW_BYTES + (c % C::CPR) * 16);
        }
    };
#include "kvz_decode_step.inc"
    // The wave's tiles, one requested AHEAD of the one being computed and the index entries one tile ahead of that; the steady-state
    // loop issues both UNCONDITIONALLY and the last tile is computed after the loop (the load structure of varlen_attn_split2_kernel).
    const int t_first = c0 + wave * TILE_KT;
    constexpr int T_STEP = RT_WAVES * TILE_KT;
    if (t_first < c1) {
        int e_next = request_pos(t_first + T_STEP);
        load_tile(kraw, vraw, position(request_pos(t_first), t_first));
        int t0 = t_first;
#pragma unroll 1
        for (; t0 + T_STEP < c1; t0 += T_STEP) {
            const int e_after = request_pos(t0 + 2 * T_STEP);
            load_tile(knext, vnext, position(e_next, t0 + T_STEP));
            compute_tile(kraw, vraw, t0);
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int kk = 0; kk < C::KK; ++kk) kraw[sub][kk] = knext[sub][kk];
#pragma unroll
            for (int it = 0; it < C::VLOADS; ++it) vraw[it] = vnext[it];
            e_next = e_after;
        }
        compute_tile(kraw, vraw, t0);
    }

    const int64_t pbase = ((int64_t)(first_item + split) * n_rtiles + rt) * TILE_RT;  // partial slot of this item
#include "kvz_decode_merge.inc"
}

// merge the partials of the key ranges.  grid = (Hkv, row tiles, 16 query rows); the body is combine_partials of kvz_combine.h.
template <typename T, int D>
__global__ __launch_bounds__(CB_THREADS) void retain_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                                   HeadMeta hm, int tail, int Hkv, int G, int q_len, int target_items,
                                                                   int n_rtiles, T* __restrict__ out) {
    const int h = blockIdx.x, rt = blockIdx.y, qq = blockIdx.z;
    const int R = q_len * G;
    if (rt * TILE_RT + qq >= R) return;
    const ItemRange ir = item_range([&](int hh) -> int { return hm.cnt[hh] + tail; }, Hkv, h, target_items);
    const int64_t base = ((int64_t)ir.first_item * n_rtiles + rt) * TILE_RT + qq;  // + s * n_rtiles * TILE_RT
    const int64_t istride = (int64_t)n_rtiles * TILE_RT;
    combine_partials<T, D>(ir.nsp, [&](int s2) -> Partial {
        const int64_t pi = base + s2 * istride;
        return Partial{part_ml + pi * 2, part_o + pi * D};
    }, out + ((int64_t)h * R + rt * TILE_RT + qq) * D);
}

template <typename T, int D>
static int launch_retain(const void* q, const void* k, const void* v, int64_t head_stride, const int32_t* idx, int64_t idx_len,
                         const int32_t* meta_host, int ctx_end, int tail, int rows, int Hkv, int G, int q_len, float scale, int causal,
                         void* out, void* ws, hipStream_t stream, const void* k_new = nullptr, const void* v_new = nullptr,
                         int64_t kn_stride = 0, int64_t vn_stride = 0) {
    const int n_rtiles = (q_len * G + TILE_RT - 1) / TILE_RT;
    const SplitWs w = split_ws(ws, Hkv, n_rtiles, D);  // (the layout of kvz_varlen_attn)
    const int target = target_items(Hkv);
    HeadMeta hm;
    for (int h = 0; h < RT_MAXH; ++h) {
        hm.start[h] = h < Hkv ? meta_host[h] : 0;
        hm.cnt[h] = h < Hkv ? meta_host[Hkv + h] : 0;
    }
    const dim3 grid(target + Hkv, n_rtiles), block(RT_THREADS);
    ProfScope ps("retain_attn", stream);
#define KVZ_RETAIN_LAUNCH(APP)                                                                                                          \
    hipLaunchKernelGGL((retain_attn_kernel<T, D, APP>), grid, block, 0, stream, reinterpret_cast<const T*>(q),                          \
                       reinterpret_cast<const T*>(k), reinterpret_cast<const T*>(v), head_stride, idx, idx_len, hm, ctx_end, tail, rows,  \
                       Hkv, G, q_len, target, scale, causal, w.part_o, w.part_ml, n_rtiles, reinterpret_cast<const T*>(k_new),            \
                       reinterpret_cast<const T*>(v_new), kn_stride, vn_stride)
    if (k_new) KVZ_RETAIN_LAUNCH(true);
    else KVZ_RETAIN_LAUNCH(false);
#undef KVZ_RETAIN_LAUNCH
    KVZ_CHECK_LAUNCH("retain_attn_kernel");
    hipLaunchKernelGGL((retain_combine_kernel<T, D>), dim3(Hkv, n_rtiles, TILE_RT), dim3(CB_THREADS), 0, stream, w.part_o, w.part_ml, hm,
                       tail, Hkv, G, q_len, target, n_rtiles, reinterpret_cast<T*>(out));
    KVZ_CHECK_LAUNCH("retain_combine_kernel");
    return KVZ_OK;
}

static int index_impl(const char* who, const uint8_t* valid, int tok1, int layers, int Hkv, int N, int sink, const int32_t* tile_base,
                      const int32_t* row_start, int32_t* idx, int64_t idx_len, kvz_stream_t stream_) {
    KVZ_REQUIRE(valid && tile_base && row_start && idx, KVZ_EINVAL, "%s: null pointer", who);
    KVZ_REQUIRE((reinterpret_cast<uintptr_t>(idx) & 3u) == 0 && (reinterpret_cast<uintptr_t>(row_start) & 3u) == 0 &&
                    (reinterpret_cast<uintptr_t>(tile_base) & 3u) == 0, KVZ_EINVAL, "%s: idx, row_start and tile_base must be 4-byte aligned", who);
    KVZ_REQUIRE(layers > 0 && Hkv > 0 && Hkv <= 65535 && (int64_t)layers * Hkv <= 65535 && layers <= 65535, KVZ_EINVAL,
                "%s: bad shape (layers %d, Hkv %d)", who, layers, Hkv);
    KVZ_REQUIRE(N >= 0 && sink >= 0 && (int64_t)sink + N > 0 && (int64_t)sink + N < ((int64_t)1 << 31) - CT, KVZ_EINVAL,
                "%s: bad context (sink %d, N %d)", who, sink, N);
    KVZ_REQUIRE(idx_len >= 0, KVZ_EINVAL, "%s: idx_len = %lld is negative", who, (long long)idx_len);
    const int nt = (sink + N + CT - 1) / CT;
    hipStream_t stream = (hipStream_t)stream_;
    ProfScope ps("retain_index", stream);
    hipLaunchKernelGGL(retain_index_kernel, dim3((unsigned)nt, (unsigned)Hkv, (unsigned)layers), dim3(IX_THREADS), 0, stream, valid, tok1,
                       Hkv, N, sink, nt, tile_base, row_start, idx, idx_len);
    KVZ_CHECK_LAUNCH("retain_index_kernel");
    return KVZ_OK;
}

}  // namespace retain
}  // namespace kvz

using namespace kvz;

extern "C" int kvz_retain_index(const uint8_t* valid, int layers, int Hkv, int N, int sink, const int32_t* tile_base,
                                const int32_t* row_start, int32_t* idx, int64_t idx_len, kvz_stream_t stream) {
    return retain::index_impl("kvz_retain_index", valid, 1, layers, Hkv, N, sink, tile_base, row_start, idx, idx_len, stream);
}
extern "C" int kvz_retain_index_heads(const uint8_t* valid_heads, int layers, int Hkv, int N, int sink, const int32_t* tile_base,
                                      const int32_t* row_start, int32_t* idx, int64_t idx_len, kvz_stream_t stream) {
    return retain::index_impl("kvz_retain_index_heads", valid_heads, 0, layers, Hkv, N, sink, tile_base, row_start, idx, idx_len, stream);
}

// query rows per head above which kvz_varlen_attn hands over to the multi-row kernel: these calls stop there
static int retain_max_rows() { return tunable(TUNE_FLASH_MIN_ROWS); }

extern "C" size_t kvz_retain_attn_workspace_bytes(int Hkv, int G, int q_len, int D) {
    if (Hkv <= 0 || G <= 0 || q_len <= 0 || D <= 0) return 0;
    if ((int64_t)q_len * G > retain_max_rows()) return 0;
    const int n_rtiles = (q_len * G + TILE_RT - 1) / TILE_RT;
    return split_ws(nullptr, Hkv, n_rtiles, D).bytes;
}

// the checks the two attention calls share; `rows` = rows of a head that are read (fill, + 1 with the append), `tail` the keys behind the
// indexed ones
static int retain_check(const char* who, const void* q, const void* k, const void* v, int64_t head_stride, int capacity, const int32_t* idx,
                        int64_t idx_len, const int32_t* meta_host, int ctx_end, int Hkv, int G, int q_len, int D, int dtype,
                        const void* out, const void* ws, size_t ws_bytes) {
    KVZ_REQUIRE(q && k && v && idx && meta_host && out && ws, KVZ_EINVAL, "%s: null pointer", who);
    KVZ_REQUIRE(Hkv > 0 && G > 0 && q_len > 0, KVZ_EINVAL, "%s: bad shape (Hkv %d, G %d, q_len %d)", who, Hkv, G, q_len);
    KVZ_REQUIRE(D == 64 || D == 128, KVZ_EUNSUPPORTED, "%s: head_dim %d unsupported (64 or 128)", who, D);
    KVZ_REQUIRE(Hkv <= retain::RT_MAXH, KVZ_EUNSUPPORTED, "%s: %d KV heads unsupported (Hkv <= %d)", who, Hkv, retain::RT_MAXH);
    KVZ_REQUIRE((int64_t)q_len * G <= retain_max_rows(), KVZ_EUNSUPPORTED,
                "%s: %d positions x %d query heads per KV head unsupported (q_len*G <= %d query rows per head: beyond, gather and "
                "kvz_flash_fwd)", who, q_len, G, retain_max_rows());
    KVZ_REQUIRE(dtype == KVZ_F16 || dtype == KVZ_BF16, KVZ_EINVAL, "%s: bad dtype %d", who, dtype);
    KVZ_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(ws) &&
                    (reinterpret_cast<uintptr_t>(idx) & 3u) == 0, KVZ_EINVAL,
                "%s: pointers must be 16-byte aligned (idx: 4 bytes)", who);
    KVZ_REQUIRE(capacity > 0 && head_stride % 8 == 0 && head_stride >= (int64_t)capacity * D, KVZ_EINVAL,
                "%s: head_stride = %lld must be a multiple of 8 elements and hold capacity = %d rows", who, (long long)head_stride, capacity);
    KVZ_REQUIRE(ctx_end >= 0, KVZ_EINVAL, "%s: ctx_end = %d is negative", who, ctx_end);
    KVZ_REQUIRE(idx_len >= 1, KVZ_EINVAL, "%s: idx_len = %lld (an index holds at least one entry)", who, (long long)idx_len);
    for (int h = 0; h < Hkv; ++h) {
        const int64_t s = meta_host[h], n = meta_host[Hkv + h];
        KVZ_REQUIRE(s >= 0 && n >= 0, KVZ_EINVAL, "%s: negative index start or count of head %d", who, h);
        KVZ_REQUIRE(n <= ctx_end && s + n <= idx_len, KVZ_EINVAL,
                    "%s: head %d indexes %lld positions from entry %lld on (ctx_end %d, idx_len %lld)", who, h, (long long)n, (long long)s,
                    ctx_end, (long long)idx_len);
    }
    KVZ_REQUIRE(ws_bytes >= kvz_retain_attn_workspace_bytes(Hkv, G, q_len, D), KVZ_EWORKSPACE, "%s: workspace too small (%zu bytes, %zu needed)",
                who, ws_bytes, kvz_retain_attn_workspace_bytes(Hkv, G, q_len, D));
    return KVZ_OK;
}

extern "C" int kvz_retain_attn(const void* q, const void* k_store, const void* v_store, int64_t head_stride, int capacity,
                               const int32_t* idx, int64_t idx_len, const int32_t* meta_host, int ctx_end, int fill, int Hkv, int G,
                               int q_len, int D, float scale, int causal, int dtype, void* out, void* ws, size_t ws_bytes,
                               kvz_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = retain_check("kvz_retain_attn", q, k_store, v_store, head_stride, capacity, idx, idx_len, meta_host, ctx_end, Hkv, G,
                                q_len, D, dtype, out, ws, ws_bytes);
    if (rc) return rc;
    KVZ_REQUIRE((int64_t)fill >= (int64_t)ctx_end + q_len, KVZ_EINVAL,
                "kvz_retain_attn: fill = %d is below ctx_end = %d plus q_len = %d: the rows of the query positions are not in the store", fill,
                ctx_end, q_len);
    KVZ_REQUIRE(fill <= capacity, KVZ_EINVAL, "kvz_retain_attn: fill = %d exceeds capacity = %d", fill, capacity);
#define KVZ_RETAIN_CALL(T, DD)                                                                                                           \
    return retain::launch_retain<T, DD>(q, k_store, v_store, head_stride, idx, idx_len, meta_host, ctx_end, fill - ctx_end, fill, Hkv, G, \
                                        q_len, scale, causal, out, ws, stream)
    KVZ_DISPATCH_HALF_D(dtype, D, KVZ_RETAIN_CALL);
#undef KVZ_RETAIN_CALL
}

extern "C" int kvz_retain_attn_append(const void* q, void* k_store, void* v_store, int64_t head_stride, int capacity, const void* k_new,
                                      const void* v_new, int64_t k_new_head_stride, int64_t v_new_head_stride, const int32_t* idx,
                                      int64_t idx_len, const int32_t* meta_host, int ctx_end, int fill, int Hkv, int G, int D, float scale,
                                      int dtype, void* out, void* ws, size_t ws_bytes, kvz_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KVZ_REQUIRE(k_new && v_new, KVZ_EINVAL, "kvz_retain_attn_append: null pointer");
    const int rc = retain_check("kvz_retain_attn_append", q, k_store, v_store, head_stride, capacity, idx, idx_len, meta_host, ctx_end, Hkv,
                                G, 1, D, dtype, out, ws, ws_bytes);
    if (rc) return rc;
    KVZ_REQUIRE(aligned16(k_new) && aligned16(v_new), KVZ_EINVAL, "kvz_retain_attn_append: pointers must be 16-byte aligned (idx: 4 bytes)");
    KVZ_REQUIRE(k_new_head_stride % 8 == 0 && v_new_head_stride % 8 == 0, KVZ_EINVAL,
                "kvz_retain_attn_append: the head strides of the new rows must be multiples of 8 elements");
    KVZ_REQUIRE(fill >= ctx_end, KVZ_EINVAL, "kvz_retain_attn_append: fill = %d is below ctx_end = %d", fill, ctx_end);
    KVZ_REQUIRE((int64_t)fill + 1 <= capacity, KVZ_EINVAL,
                "kvz_retain_attn_append: fill = %d plus the new row exceeds capacity = %d: grow the store first", fill, capacity);
#define KVZ_RETAIN_CALL(T, DD)                                                                                                         \
    return retain::launch_retain<T, DD>(q, k_store, v_store, head_stride, idx, idx_len, meta_host, ctx_end, fill - ctx_end + 1, fill + 1, \
                                        Hkv, G, 1, scale, 1, out, ws, stream, k_new, v_new, k_new_head_stride, v_new_head_stride)
    KVZ_DISPATCH_HALF_D(dtype, D, KVZ_RETAIN_CALL);
#undef KVZ_RETAIN_CALL
}
