// kvz_attn.hip — variable-length (ragged per KV head) post-prune attention for gfx950.
//
// Replaces the reference's call into flash_attn_varlen_func (attention/attn.py:56-73; flash-attn
// 2.7.4.post1, third party, not vendored): every KV head is one ragged "sequence", its G query heads
// are MQA heads, causal mask bottom-right aligned.
//
// Decode (q_len = 1) is HBM-bound: every kept K and V row is read exactly once per generated token.
// Design: split-K "flash decoding" in ONE launch.
//   grid = (work items, row tiles of 16 query rows); a block owns one key range of one head (ranges are cut from the SUM of
//   the ragged head lengths), its 8 waves stride over 32-key tiles of the range.
//   S^T = K.Q^T on v_mfma_f32_16x16x32 with K rows loaded straight from HBM as the A operand (16-byte
//   contiguous per lane, no LDS); softmax state lives in registers (lane = one query row);
//   O^T += V^T.P^T with V staged through a per-wave padded LDS tile and read back transposed by
//   ds_read_b64_tr_b16 (types and tile constants: kvz_wave_tile.h).  A second kernel merges the head's partials.
#include "kvz_combine.h"

namespace kvz {

constexpr int AT_THREADS = 512;
constexpr int AT_WAVES = 8;

// APPEND: the decode step's O(1) cache append is done by the attention kernel.  k_len_offset already counts the new token; the
// block that owns the last key range of a head first copies the new K and V row of that head from the state tensors into
// the cache (row k_start[h] + len - 1) and then reads it back like any other key (no other block touches that row).

// ---- round 2: ragged-aware work items -------------------------------------------------------------------------------------
// Work items are cut from the SUM of the head lengths (a head of 120 k keys gets 30 x the items of a head of 4 k keys; a
// dropped head of a head-level cache gets one), not from Hkv x the longest head: every block derives its (head, key range)
// from the lengths (kernel arguments when the host knows them, else scalar loads).  The partials of a head are merged by a
// second, split-parallel kernel.  (Merging them inside this kernel - last block of a head to arrive, write-through partials,
// one device-scope counter, one acquire fence - was built and measured in round 2: correct, but the chain store drain ->
// atomic -> fence -> two dependent rounds of reads costs 10-12 us of serial tail against 5.4 + 2 us for the separate launch;
// see profiles/r2_attn_fused_vs_split.txt.)
constexpr int AT_MAXH = 64;
struct HeadMeta { int32_t start[AT_MAXH]; int32_t len[AT_MAXH]; };

template <typename T, int D, bool APPEND, bool HOSTMETA>
__global__ __launch_bounds__(AT_THREADS) void varlen_attn_split2_kernel(
    const T* __restrict__ q, const T* k, const T* v, const int32_t* __restrict__ k_start, const int32_t* __restrict__ k_len,
    int k_len_offset, const int32_t* __restrict__ k_len_offset_dev, HeadMeta hm, int Hkv, int G, int q_len, int target_items, float scale,
    int causal, float* part_o, float* part_ml, uint32_t* counters, int n_rtiles, T* __restrict__ out, const T* __restrict__ k_new,
    const T* __restrict__ v_new, int64_t kn_head_stride, int64_t vn_head_stride) {
    typedef TileCfg<D> C;
    typedef typename Half<T>::v8 v8;
    // (the part of the appended-token count that lives on the DEVICE: a captured generation step is replayed with unchanged arguments)
    if (k_len_offset_dev) k_len_offset += *k_len_offset_dev;
    auto len_of = [&](int hh) -> int { return (HOSTMETA ? hm.len[hh] : k_len[hh]) + k_len_offset; };
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
    const int64_t seg = HOSTMETA ? hm.start[h] : k_start[h];
    const int c0 = split * chunk;
    const int c1 = min(len, c0 + chunk);
    if (APPEND && c1 == len) {
        constexpr int CH = D * 2 / 16;  // 16-byte chunks per row
        if ((int)threadIdx.x < 2 * CH) {
            const bool is_v = (int)threadIdx.x >= CH;
            const int c = (int)threadIdx.x - (is_v ? CH : 0);
            const char* src = reinterpret_cast<const char*>(is_v ? v_new + h * vn_head_stride : k_new + h * kn_head_stride) + c * 16;
            char* dst = const_cast<char*>(reinterpret_cast<const char*>(is_v ? v : k)) + (seg + len - 1) * (D * 2) + c * 16;
            *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
        }
        __syncthreads();  // (workgroup-scope release/acquire: the row is visible to the loads of this block below)
    }
    const int R = q_len * G;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int l15 = lane & 15, quad = lane >> 4;

    constexpr int BLOCK_WAVES = AT_WAVES;
    __shared__ __attribute__((aligned(16))) char lds[AT_WAVES * C::WAVE_LDS];
    char* wl = lds + wave * C::WAVE_LDS;

    const int n_qrows = R;
    const int64_t q_row0 = (int64_t)h * R;
#include "kvz_decode_state.inc"
    int limit = causal ? (qrow / G) + len - q_len : len - 1;  // last visible key of this lane's query row (bottom-right aligned)
    if (!qvalid) limit = -1;
    auto visible = [&](int key) -> bool { return key <= limit && key < c1; };
    // (behind `limit`, where they always stood: the order of a kernel's statements is part of what the compiler sees)
    const char* kbase = reinterpret_cast<const char*>(k) + seg * C::ROW_BYTES;
    const char* vbase = reinterpret_cast<const char*>(v) + seg * C::ROW_BYTES;
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

    const int64_t pbase = ((int64_t)(first_item + split) * n_rtiles + rt) * TILE_RT;  // partial slot of this item
#include "kvz_decode_merge.inc"
}

// merge the partials of the key ranges.  grid = (Hkv, row tiles, 16 query rows); the body is combine_partials of kvz_combine.h.
template <typename T, int D, bool HOSTMETA>
__global__ __launch_bounds__(CB_THREADS) void varlen_attn_combine2_kernel(const float* __restrict__ part_o,
                                                                         const float* __restrict__ part_ml,
                                                                         const int32_t* __restrict__ k_len, int k_len_offset,
                                                                         const int32_t* __restrict__ k_len_offset_dev,
                                                                         HeadMeta hm, int Hkv, int G, int q_len, int target_items,
                                                                         int n_rtiles, T* __restrict__ out) {
    if (k_len_offset_dev) k_len_offset += *k_len_offset_dev;
    const int h = blockIdx.x, rt = blockIdx.y, qq = blockIdx.z;
    const int R = q_len * G;
    if (rt * TILE_RT + qq >= R) return;
    const ItemRange ir = item_range([&](int hh) -> int { return (HOSTMETA ? hm.len[hh] : k_len[hh]) + k_len_offset; }, Hkv, h,
                                    target_items);
    const int64_t base = ((int64_t)ir.first_item * n_rtiles + rt) * TILE_RT + qq;  // + s * n_rtiles * TILE_RT
    const int64_t istride = (int64_t)n_rtiles * TILE_RT;
    combine_partials<T, D>(ir.nsp, [&](int s2) -> Partial {
        const int64_t pi = base + s2 * istride;
        return Partial{part_ml + pi * 2, part_o + pi * D};
    }, out + ((int64_t)h * R + rt * TILE_RT + qq) * D);
}

__global__ void add_i32_kernel(int32_t* p, int delta) { *p += delta; }

template <typename T, int D>
static int launch_attn(const void* q, const void* k, const void* v, const int32_t* k_start, const int32_t* k_len,
                       int k_len_offset, const int32_t* off_dev, const int32_t* meta_host, int Hkv, int G, int q_len, float scale, int causal, void* out,
                       void* ws, hipStream_t stream, const void* k_new = nullptr, const void* v_new = nullptr,
                       int64_t kn_stride = 0, int64_t vn_stride = 0) {
    const int n_rtiles = (q_len * G + TILE_RT - 1) / TILE_RT;
    const SplitWs w = split_ws(ws, Hkv, n_rtiles, D);
    const int target = target_items(Hkv);
    HeadMeta hm;
    const bool host = meta_host != nullptr && Hkv <= AT_MAXH;
    if (host)
        for (int h = 0; h < Hkv; ++h) { hm.start[h] = meta_host[h]; hm.len[h] = meta_host[Hkv + h]; }
    const dim3 grid(target + Hkv, n_rtiles), block(AT_THREADS);
    ProfScope ps("varlen_attn", stream);
#define KVZ_ATTN_LAUNCH(APP, HOST)                                                                                                \
    hipLaunchKernelGGL((varlen_attn_split2_kernel<T, D, APP, HOST>), grid, block, 0, stream, reinterpret_cast<const T*>(q),          \
                       reinterpret_cast<const T*>(k), reinterpret_cast<const T*>(v), k_start, k_len, k_len_offset, off_dev, hm, Hkv, G, \
                       q_len, target, scale, causal, w.part_o, w.part_ml, w.counters, n_rtiles, reinterpret_cast<T*>(out),          \
                       reinterpret_cast<const T*>(k_new), reinterpret_cast<const T*>(v_new), kn_stride, vn_stride)
    if (k_new) { if (host) KVZ_ATTN_LAUNCH(true, true); else KVZ_ATTN_LAUNCH(true, false); }
    else { if (host) KVZ_ATTN_LAUNCH(false, true); else KVZ_ATTN_LAUNCH(false, false); }
#undef KVZ_ATTN_LAUNCH
    KVZ_CHECK_LAUNCH("varlen_attn_split2_kernel");
    const dim3 cgrid(Hkv, n_rtiles, TILE_RT), cblock(CB_THREADS);
    if (host)
        hipLaunchKernelGGL((varlen_attn_combine2_kernel<T, D, true>), cgrid, cblock, 0, stream, w.part_o, w.part_ml, k_len, k_len_offset,
                           off_dev, hm, Hkv, G, q_len, target, n_rtiles, reinterpret_cast<T*>(out));
    else
        hipLaunchKernelGGL((varlen_attn_combine2_kernel<T, D, false>), cgrid, cblock, 0, stream, w.part_o, w.part_ml, k_len, k_len_offset,
                           off_dev, hm, Hkv, G, q_len, target, n_rtiles, reinterpret_cast<T*>(out));
    KVZ_CHECK_LAUNCH("varlen_attn_combine2_kernel");
    return KVZ_OK;
}

}  // namespace kvz

using namespace kvz;

// query rows per head above which the multi-row kernel takes over from the split-key decode kernel
static int flash_min_rows() { return tunable(TUNE_FLASH_MIN_ROWS); }

extern "C" size_t kvz_varlen_attn_workspace_bytes(int Hkv, int G, int q_len, int D, int max_len_k) {
    if (Hkv <= 0 || G <= 0 || q_len <= 0 || D <= 0 || max_len_k < 0) return 0;
    if (q_len * G > flash_min_rows()) return kvz_flash_workspace_bytes(Hkv, G, q_len, D) + 256;  // (never 0: callers pass a buffer)
    const int n_rtiles = (q_len * G + TILE_RT - 1) / TILE_RT;
    return split_ws(nullptr, Hkv, n_rtiles, D).bytes;
}

extern "C" int kvz_varlen_attn(const void* q, const void* k, const void* v, const int32_t* k_start,
                               const int32_t* k_len, int k_len_offset, const int32_t* k_len_offset_dev, const int32_t* k_meta_host, int Hkv, int G, int q_len,
                               int D, int max_len_k, float scale,
                               int causal, int dtype, void* out, void* ws, size_t ws_bytes, kvz_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KVZ_REQUIRE(q && k && v && k_start && k_len && out && ws, KVZ_EINVAL, "kvz_varlen_attn: null pointer");
    KVZ_REQUIRE(Hkv > 0 && Hkv <= 65535 && G > 0 && q_len > 0 && max_len_k >= 0, KVZ_EINVAL, "kvz_varlen_attn: bad shape");
    KVZ_REQUIRE(D == 64 || D == 128, KVZ_EUNSUPPORTED, "kvz_varlen_attn: head_dim %d unsupported (64 or 128)", D);
    KVZ_REQUIRE(dtype == KVZ_F16 || dtype == KVZ_BF16, KVZ_EINVAL, "kvz_varlen_attn: bad dtype %d", dtype);
    KVZ_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(ws), KVZ_EINVAL,
                "kvz_varlen_attn: q/k/v/ws must be 16-byte aligned");
    if (q_len * G > flash_min_rows()) {  // many query rows: one pass over the keys per 128-row block (kvz_flash.hip)
        KVZ_REQUIRE(k_len_offset_dev == nullptr, KVZ_EUNSUPPORTED, "kvz_varlen_attn: a device-side offset is a decode-step feature (q_len*G <= %d rows)", flash_min_rows());
        KVZ_REQUIRE(ws_bytes >= kvz_varlen_attn_workspace_bytes(Hkv, G, q_len, D, max_len_k), KVZ_EWORKSPACE,
                    "kvz_varlen_attn: workspace too small");
        return kvz_flash_fwd(q, (int64_t)q_len * G * D, D, (int64_t)G * D, k, v, k_start, k_len, k_len_offset, k_meta_host, Hkv, G,
                             q_len, D, scale, causal, dtype, out, (int64_t)q_len * G * D, D, (int64_t)G * D, nullptr, ws, ws_bytes,
                             stream_);
    }
    KVZ_REQUIRE((q_len * G + TILE_RT - 1) / TILE_RT <= 65535, KVZ_EINVAL, "kvz_varlen_attn: too many query rows");
    KVZ_REQUIRE(ws_bytes >= kvz_varlen_attn_workspace_bytes(Hkv, G, q_len, D, max_len_k), KVZ_EWORKSPACE,
                "kvz_varlen_attn: workspace too small");
#define KVZ_ATTN_CALL(T, DD) \
    return launch_attn<T, DD>(q, k, v, k_start, k_len, k_len_offset, k_len_offset_dev, k_meta_host, Hkv, G, q_len, scale, causal, out, ws, stream)
    KVZ_DISPATCH_HALF_D(dtype, D, KVZ_ATTN_CALL);
#undef KVZ_ATTN_CALL
}

extern "C" int kvz_varlen_attn_append(const void* q, void* k_cache, void* v_cache, const void* k_state, const void* v_state,
                                      int64_t k_state_head_stride, int64_t v_state_head_stride, const int32_t* k_start,
                                      const int32_t* k_len, int k_len_offset, const int32_t* k_len_offset_dev,
                                      const int32_t* k_meta_host, int Hkv, int G, int D, int max_len_k, float scale, int dtype, void* out,
                                      void* ws, size_t ws_bytes, kvz_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KVZ_REQUIRE(q && k_cache && v_cache && k_state && v_state && k_start && k_len && out && ws, KVZ_EINVAL,
                "kvz_varlen_attn_append: null pointer");
    KVZ_REQUIRE(Hkv > 0 && Hkv <= 65535 && G > 0 && max_len_k >= 1 && k_len_offset >= 0, KVZ_EINVAL, "kvz_varlen_attn_append: bad shape");
    KVZ_REQUIRE(D == 64 || D == 128, KVZ_EUNSUPPORTED, "kvz_varlen_attn_append: head_dim %d unsupported (64 or 128)", D);
    KVZ_REQUIRE(dtype == KVZ_F16 || dtype == KVZ_BF16, KVZ_EINVAL, "kvz_varlen_attn_append: bad dtype %d", dtype);
    KVZ_REQUIRE(aligned16(q) && aligned16(k_cache) && aligned16(v_cache) && aligned16(k_state) && aligned16(v_state) && aligned16(ws),
                KVZ_EINVAL, "kvz_varlen_attn_append: pointers must be 16-byte aligned");
    KVZ_REQUIRE((k_state_head_stride * 2) % 16 == 0 && (v_state_head_stride * 2) % 16 == 0, KVZ_EINVAL,
                "kvz_varlen_attn_append: state head strides must be multiples of 8 elements");
    KVZ_REQUIRE(ws_bytes >= kvz_varlen_attn_workspace_bytes(Hkv, G, 1, D, max_len_k), KVZ_EWORKSPACE,
                "kvz_varlen_attn_append: workspace too small");
    const int off = k_len_offset + 1;  // the keys attended to include the token appended by this call
#define KVZ_ATTN_CALL(T, DD)                                                                                                          \
    return launch_attn<T, DD>(q, k_cache, v_cache, k_start, k_len, off, k_len_offset_dev, k_meta_host, Hkv, G, 1, scale, 1, out, ws, stream, \
                              k_state, v_state, k_state_head_stride, v_state_head_stride)
    KVZ_DISPATCH_HALF_D(dtype, D, KVZ_ATTN_CALL);
#undef KVZ_ATTN_CALL
}


// the device-side part of the appended-token count (k_len_offset_dev of the attention calls): += delta, one tiny launch - the last
// node of a captured generation step
extern "C" int kvz_add_i32(int32_t* p, int delta, kvz_stream_t stream_) {
    KVZ_REQUIRE(p && (reinterpret_cast<uintptr_t>(p) & 3u) == 0, KVZ_EINVAL, "kvz_add_i32: bad pointer");
    hipLaunchKernelGGL(add_i32_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream_, p, delta);
    KVZ_CHECK_LAUNCH("add_i32_kernel");
    return KVZ_OK;
}
