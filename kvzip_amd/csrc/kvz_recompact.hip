// kvz_recompact.hip — tighten a pruned cache: gather the ragged (already compacted) layout into a smaller one (gfx950).
//
// EvictCache.tighten: a cache pruned with mask `old` is pruned again with a mask `new` that is a subset of it (a smaller ratio of the
// same scores).  Every row `new` keeps is still in the flat cache, so nothing dense is needed: per (layer, head, 1024-token tile) the
// rows the OLD mask kept form one contiguous run that starts at  old_seg_start + old_tile_base[tile],  and the row of position p inside
// that run is the OLD RANK of p (old mask bits before p in the tile).  The block builds the list of old ranks of the positions the NEW
// mask keeps and copies them, in order, to  new_seg_start + new_tile_base[tile] ...  - the copy loop of compact_gather_kernel
// (kvz_compact.hip): row_bytes / 16 lanes per row, 16-byte non-temporal loads and stores, K and V in one block, 8 rows in flight per
// lane group.  Destination rows are consecutive, source rows an increasing subsequence of a contiguous run.
//
// One more block per (layer, head) carries the rows appended after the prune (query / answer K,V of a multi-turn generation, which sit
// behind the head's rows in its slack).  Out of place only: outputs are fresh buffers (an in-place variant would need ordering between
// blocks).  Algorithmic bytes: those of a fresh compaction at the new mask + one more mask read.
#include "kvz_common.h"
#include "../../include/kvzip_hip_tighten.h"

namespace kvz {

constexpr int RT = KVZ_COMPACT_TILE;  // tokens per tile (the tile of both plans)
constexpr int RC_THREADS = 256;
constexpr int RC_PER_THREAD = RT / RC_THREADS;
static_assert(RC_PER_THREAD == 4, "tile/threads layout");

typedef uint32_t rc_u32x4 __attribute__((ext_vector_type(4)));

struct RecompactArgs {
    const void* const* k_ptrs;   // device pointer tables, one flat [rows, D] buffer per layer
    const void* const* v_ptrs;
    void* const* k_out_ptrs;
    void* const* v_out_ptrs;
    const uint8_t* old_valid;    // [layers*Hkv, N]  (tok1 = 0: [layers*Hkv])
    const uint8_t* new_valid;
    int old_tok1, new_tok1;
    const int32_t* old_tile_base;  // [layers*Hkv, ntiles]
    const int32_t* old_seg_start;  // [layers*Hkv]
    const int32_t* old_len_k;
    const int32_t* new_tile_base;
    const int32_t* new_seg_start;
    const int32_t* new_len_k;
    const int32_t* tail_rows;      // [layers] or nullptr
    int Hkv, N, sink, klen, ntiles;
    int row_bytes;                 // D * elem_bytes
};

// LPR = lanes per row = row_bytes / 16 (power of two, 4..64).  grid (ntiles + 1, Hkv, layers)
template <int LPR>
__global__ __launch_bounds__(RC_THREADS) void recompact_gather_kernel(RecompactArgs a) {
    const int tile = blockIdx.x;
    const int h = blockIdx.y;
    const int layer = blockIdx.z;
    const int row = layer * a.Hkv + h;

    const char* ksrc = reinterpret_cast<const char*>(a.k_ptrs[layer]);
    const char* vsrc = reinterpret_cast<const char*>(a.v_ptrs[layer]);
    char* kdst = reinterpret_cast<char*>(a.k_out_ptrs[layer]);
    char* vdst = reinterpret_cast<char*>(a.v_out_ptrs[layer]);

    if (tile == a.ntiles) {
        // rows appended after the prune: behind the head's old rows -> behind its new rows
        const int t = a.tail_rows ? a.tail_rows[layer] : 0;
        if (t <= 0) return;
        const int64_t so = ((int64_t)a.old_seg_start[row] + a.old_len_k[row]) * a.row_bytes;
        const int64_t dof = ((int64_t)a.new_seg_start[row] + a.new_len_k[row]) * a.row_bytes;
        const int chunks = t * LPR;  // (t <= slack and LPR <= 64: far below 2^31)
        for (int i = threadIdx.x; i < chunks; i += RC_THREADS) {
            const int64_t o = (int64_t)i * 16;
            const rc_u32x4 kk = __builtin_nontemporal_load(reinterpret_cast<const rc_u32x4*>(ksrc + so + o));
            const rc_u32x4 vv = __builtin_nontemporal_load(reinterpret_cast<const rc_u32x4*>(vsrc + so + o));
            __builtin_nontemporal_store(kk, reinterpret_cast<rc_u32x4*>(kdst + dof + o));
            __builtin_nontemporal_store(vv, reinterpret_cast<rc_u32x4*>(vdst + dof + o));
        }
        return;
    }

    __shared__ uint16_t list[RT];
    __shared__ int wtot_o[RC_THREADS / WAVE];
    __shared__ int wtot_n[RC_THREADS / WAVE];

    const uint8_t* orow = a.old_valid + (int64_t)row * (a.old_tok1 ? a.N : 1);
    const uint8_t* nrow = a.new_valid + (int64_t)row * (a.new_tok1 ? a.N : 1);
    const int p0 = tile * RT + threadIdx.x * RC_PER_THREAD;
    const uint32_t ob = full_mask4(orow, p0, a.sink, a.N, a.klen, a.old_tok1);
    // a position the old mask evicted has no row any more: it cannot come back (kvz_mask_resurrects counts such requests; masking
    // here keeps every source index inside the tile's run whatever the caller passed)
    const uint32_t nb = full_mask4(nrow, p0, a.sink, a.N, a.klen, a.new_tok1) & ob;
    const int co = __popc(ob), cn = __popc(nb);
    const int inc_o = wave_inclusive_scan(co);
    const int inc_n = wave_inclusive_scan(cn);
    if (lane_id() == 63) {
        wtot_o[threadIdx.x >> 6] = inc_o;
        wtot_n[threadIdx.x >> 6] = inc_n;
    }
    __syncthreads();
    int pre_o = 0, pre_n = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) {
        pre_o += wtot_o[w];
        pre_n += wtot_n[w];
    }
    const int total = wtot_n[0] + wtot_n[1] + wtot_n[2] + wtot_n[3];
    int rank = pre_o + inc_o - co;  // old rank of position p0 inside the tile
    int o = pre_n + inc_n - cn;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (nb & (1u << j)) list[o++] = (uint16_t)rank;
        rank += (ob >> j) & 1u;
    }
    __syncthreads();
    if (total == 0) return;

    const int64_t src_row0 = (int64_t)a.old_seg_start[row] + a.old_tile_base[(int64_t)row * a.ntiles + tile];
    const int64_t dst_row0 = (int64_t)a.new_seg_start[row] + a.new_tile_base[(int64_t)row * a.ntiles + tile];
    ksrc += src_row0 * a.row_bytes;
    vsrc += src_row0 * a.row_bytes;
    kdst += dst_row0 * a.row_bytes;
    vdst += dst_row0 * a.row_bytes;

    constexpr int RPI = RC_THREADS / LPR;  // rows per block-iteration
    const int rsub = threadIdx.x / LPR;
    const int coff = (threadIdx.x % LPR) * 16;
    constexpr int UNROLL = 8;
    for (int j0 = 0; j0 < total; j0 += RPI * UNROLL) {
        rc_u32x4 kv[UNROLL], vv[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int j = j0 + u * RPI + rsub;
            if (j < total) {
                const int64_t so = (int64_t)list[j] * a.row_bytes + coff;
                // streamed exactly once: non-temporal
                kv[u] = __builtin_nontemporal_load(reinterpret_cast<const rc_u32x4*>(ksrc + so));
                vv[u] = __builtin_nontemporal_load(reinterpret_cast<const rc_u32x4*>(vsrc + so));
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int j = j0 + u * RPI + rsub;
            if (j < total) {
                const int64_t dof = (int64_t)j * a.row_bytes + coff;
                __builtin_nontemporal_store(kv[u], reinterpret_cast<rc_u32x4*>(kdst + dof));
                __builtin_nontemporal_store(vv[u], reinterpret_cast<rc_u32x4*>(vdst + dof));
            }
        }
    }
}

// ---- positions the new mask keeps although the old one evicted them ---------------------------------
// one block per (row, chunk of RS_CHUNK positions); block reduction, ONE atomic add per block that found any
constexpr int RS_ITERS = 4;
constexpr int RS_CHUNK = RT * RS_ITERS;
__global__ __launch_bounds__(RC_THREADS) void mask_resurrects_kernel(const uint8_t* __restrict__ new_valid, int new_tok1,
                                                                    const uint8_t* __restrict__ old_valid, int old_tok1, int N,
                                                                    int nchunks, int32_t* __restrict__ count) {
    const int64_t row = blockIdx.x / nchunks;
    const int chunk = blockIdx.x % nchunks;
    const uint8_t* nrow = new_valid + row * (new_tok1 ? N : 1);
    const uint8_t* orow = old_valid + row * (old_tok1 ? N : 1);
    int c = 0;
#pragma unroll
    for (int it = 0; it < RS_ITERS; ++it) {
        const int p0 = chunk * RS_CHUNK + it * RT + threadIdx.x * RC_PER_THREAD;
        if (p0 < N) {  // (sink = 0, klen = N: bits from N on are 0 in both)
            const uint32_t nb = full_mask4(nrow, p0, 0, N, N, new_tok1);
            const uint32_t ob = full_mask4(orow, p0, 0, N, N, old_tok1);
            c += __popc(nb & ~ob);
        }
    }
    __shared__ int ws[RC_THREADS / WAVE];
    const int w = wave_reduce_sum(c);
    if (lane_id() == 0) ws[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int tot = ws[0] + ws[1] + ws[2] + ws[3];
        if (tot) atomicAdd(count, tot);
    }
}

}  // namespace kvz

using namespace kvz;

extern "C" int kvz_mask_resurrects(const uint8_t* new_valid, int new_tok1, const uint8_t* old_valid, int old_tok1, int64_t rows,
                                   int N, int32_t* count, kvz_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KVZ_REQUIRE(new_valid && old_valid && count, KVZ_EINVAL, "kvz_mask_resurrects: null pointer");
    KVZ_REQUIRE(rows > 0 && N > 0, KVZ_EINVAL, "kvz_mask_resurrects: bad shape (rows %lld, N %d)", (long long)rows, N);
    KVZ_REQUIRE((reinterpret_cast<uintptr_t>(count) & 3u) == 0, KVZ_EINVAL, "kvz_mask_resurrects: count must be 4-byte aligned");
    const int nchunks = (N + RS_CHUNK - 1) / RS_CHUNK;
    KVZ_REQUIRE(rows * nchunks <= 0x7FFFFFFFll, KVZ_EINVAL, "kvz_mask_resurrects: too many rows");
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t), stream);
    KVZ_REQUIRE(e == hipSuccess, KVZ_ELAUNCH, "kvz_mask_resurrects: memset failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(mask_resurrects_kernel, dim3((unsigned)(rows * nchunks)), dim3(RC_THREADS), 0, stream, new_valid,
                       new_tok1 ? 1 : 0, old_valid, old_tok1 ? 1 : 0, N, nchunks, count);
    KVZ_CHECK_LAUNCH("mask_resurrects_kernel");
    return KVZ_OK;
}

extern "C" int kvz_recompact_layers(const void* const* k_ptrs, const void* const* v_ptrs, const uint8_t* old_valid, int old_tok1,
                                    const int32_t* old_tile_base, const int32_t* old_seg_start, const int32_t* old_len_k,
                                    const uint8_t* new_valid, int new_tok1, const int32_t* new_tile_base,
                                    const int32_t* new_seg_start, const int32_t* new_len_k, const int32_t* tail_rows, int layers,
                                    int Hkv, int N, int sink, int klen, int D, int elem_bytes, void* const* k_out_ptrs,
                                    void* const* v_out_ptrs, kvz_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KVZ_REQUIRE(k_ptrs && v_ptrs && old_valid && old_tile_base && old_seg_start && old_len_k && new_valid && new_tile_base &&
                    new_seg_start && new_len_k && k_out_ptrs && v_out_ptrs,
                KVZ_EINVAL, "kvz_recompact_layers: null pointer");
    KVZ_REQUIRE(layers > 0 && layers <= 65535 && Hkv > 0 && Hkv <= 65535 && N > 0 && sink >= 0, KVZ_EINVAL,
                "kvz_recompact_layers: bad shape (layers %d, Hkv %d, N %d, sink %d)", layers, Hkv, N, sink);
    KVZ_REQUIRE(klen >= sink + N, KVZ_EINVAL, "kvz_recompact_layers: klen %d < sink %d + N %d", klen, sink, N);
    KVZ_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4, KVZ_EINVAL, "kvz_recompact_layers: bad elem_bytes %d",
                elem_bytes);
    const int rb = D * elem_bytes;
    KVZ_REQUIRE(D > 0 && rb % 16 == 0 && rb >= 64 && rb <= 1024 && (rb & (rb - 1)) == 0, KVZ_EINVAL,
                "kvz_recompact_layers: D*elem_bytes = %d must be a power of two in [64,1024]", rb);
    RecompactArgs a{};
    a.k_ptrs = k_ptrs; a.v_ptrs = v_ptrs; a.k_out_ptrs = k_out_ptrs; a.v_out_ptrs = v_out_ptrs;
    a.old_valid = old_valid; a.new_valid = new_valid; a.old_tok1 = old_tok1 ? 1 : 0; a.new_tok1 = new_tok1 ? 1 : 0;
    a.old_tile_base = old_tile_base; a.old_seg_start = old_seg_start; a.old_len_k = old_len_k;
    a.new_tile_base = new_tile_base; a.new_seg_start = new_seg_start; a.new_len_k = new_len_k;
    a.tail_rows = tail_rows;
    a.Hkv = Hkv; a.N = N; a.sink = sink; a.klen = klen; a.ntiles = (klen + RT - 1) / RT;
    a.row_bytes = rb;
    dim3 grid((unsigned)a.ntiles + 1, (unsigned)Hkv, (unsigned)layers);
    dim3 block(RC_THREADS);
    ProfScope ps("recompact_gather", stream);
    switch (rb / 16) {
        case 4: hipLaunchKernelGGL(recompact_gather_kernel<4>, grid, block, 0, stream, a); break;
        case 8: hipLaunchKernelGGL(recompact_gather_kernel<8>, grid, block, 0, stream, a); break;
        case 16: hipLaunchKernelGGL(recompact_gather_kernel<16>, grid, block, 0, stream, a); break;
        case 32: hipLaunchKernelGGL(recompact_gather_kernel<32>, grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL(recompact_gather_kernel<64>, grid, block, 0, stream, a); break;
    }
    KVZ_CHECK_LAUNCH("recompact_gather_kernel");
    return KVZ_OK;
}
