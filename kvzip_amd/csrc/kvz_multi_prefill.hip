// kvz_multi_prefill.hip — the packed first step over B INDEPENDENT pruned caches: the query tokens of all caches of a wave in one
// split launch and one combine launch, gfx950 (ABI and semantics: include/kvzip_hip_multi_prefill.h).
//
// No reference counterpart (batch is hard-wired to 1 there).  The queries of B caches lie back to back in one packed sequence of
// T = cu_q[B] positions; cache b (own flat K and V, slack layout) owns positions cu_q[b] .. cu_q[b + 1] - 1 and S = B * Hkv ragged
// segments take part.  The work-item scheme of kvz_multi.hip with the row tiles and the in-run causal mask of kvz_fork_prefill.hip:
//   multi_prefill_split_kernel    one block per work item = (segment s = b * Hkv + h, group of MP_WAVES 16-row tiles of the run's
//                                 n_b * G query rows, row = p * G + g, part).  The parts of a (segment, group):
//                                   key ranges   `chunk` keys each of the segment's old = len + offset rows; chunk is cut from the sum
//                                                over all (segment, group) pairs of the old lengths, in multiples of 128 keys, so that
//                                                about attn_items items come out WHATEVER the number of row groups is: a wave of long
//                                                queries gets longer key ranges, not more blocks (at most target + RG items, RG the
//                                                number of (segment, group) pairs);
//                                   the triangle the run's own n_b new rows, read from k_new / v_new - never from the slack rows this
//                                                call writes, so no block waits for another block's write.  Row (p, g)
//                                                sees new rows 0 .. p: key tiles above the diagonal of a wave's rows are never
//                                                visited, the tile on it is masked per element.  One such item per (segment, group).
//                                 A WAVE owns one row tile and walks the item's keys alone, 32 at a time (no barrier, no LDS shared
//                                 between waves): S^T = K.Q^T on v_mfma_f32_16x16x32 with the K fragments straight from memory,
//                                 O^T += V^T.P^T with V through a padded per-wave LDS tile read back transposed, softmax state in
//                                 fp32 in the exp2 domain.  Partials (m, l, a[D]) in fp32 to the workspace, slot (item, row of group).
//                                 The triangle item of group 0 of every participating segment copies the n_b new rows into the slack
//                                 of cache b (16-byte vector stores); nobody reads them in this call.
//   multi_prefill_combine_kernel  per (head, packed position): merges the partials of the row's (segment, group) and writes
//                                 out = fp16/bf16(a / l), the 'div' form of kvz_multi.hip's combine.
// Tables: K,V base pointers and offsets per cache, cu_q, start, base length and FIRST WORK ITEM per segment travel BY VALUE as kernel
// arguments (1928 bytes of table, 2.0 KB of the 4 KB there are with the other arguments).  A block finds its segment with wave-uniform
// scalar work from the item prefixes (kvz_multi.hip's prefix count, up to 127 compares), then group and part by two divisions.
#include "kvz_wave_tile.h"
#include "../../include/kvzip_hip_multi_prefill.h"

#include <limits.h>

namespace kvz {
namespace mprefill {

constexpr int MP_WAVES = 4;          // row tiles of one block (one wave each, one wave per SIMD)
constexpr int MP_THREADS = MP_WAVES * WAVE;
constexpr int MP_GROUP = MP_WAVES * TILE_RT;   // query rows of a work item = partial slots of an item
constexpr int MP_MAXB = 16;          // caches
constexpr int MP_MAXH = 64;          // KV heads
constexpr int MP_MAXS = 128;         // segments: B * Hkv
constexpr int MP_MAXG = 64;          // query heads per KV head
constexpr int MP_SCAN = 16;          // prefix entries compared per batch of scalar loads

// the tables, by value.  Segment s = b * Hkv + h.  Work items are numbered segment after segment, inside a segment group after group,
// inside a group the key ranges and then the triangle: segment s owns items item0[s] .. item0[s + 1] - 1 (none when n_b = 0).
struct Table {
    void* k[MP_MAXB];                      // flat [rows, D] buffers of cache b
    void* v[MP_MAXB];
    int32_t off[MP_MAXB];                  // rows appended before this call
    int32_t cu_q[MP_MAXB + 1];             // first packed position of cache b; cu_q[b >= B] = T
    int32_t start[MP_MAXS];                // first row of segment s
    int32_t len[MP_MAXS];                  // base length of segment s (old = len + off)
    int32_t item0[MP_MAXS + 1];            // first item of segment s; item0[S] = all items, INT_MAX behind (the scan reads in batches)
};

__device__ __host__ static inline int groups_of(int n_b, int G) {
    return ((n_b * G + TILE_RT - 1) / TILE_RT + MP_WAVES - 1) / MP_WAVES;
}

template <typename T, int D>
__global__ __launch_bounds__(MP_THREADS) void multi_prefill_split_kernel(
    const T* __restrict__ q, int64_t qs_head, int64_t qs_group, int64_t qs_pos, Table tb, const T* __restrict__ k_new,
    const T* __restrict__ v_new, int64_t kn_h, int64_t kn_p, int64_t vn_h, int64_t vn_p, int S, int Hkv, int G, int chunk, float scale,
    float* __restrict__ part_o, float* __restrict__ part_ml) {
    typedef TileCfg<D> C;
    typedef typename Half<T>::v8 v8;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int l15 = lane & 15, quad = lane >> 4;

    // ---- this block's work item: (cache, head, row-tile group, part) from the item prefixes (all block-uniform scalar work) ----
    const int bx = blockIdx.x;             // (the grid has exactly as many blocks as there are items)
    int s = 0;             // the last segment whose first item is not beyond bx (segments without items share the next one's)
#pragma unroll
    for (int c = 0; c < MP_MAXS / MP_SCAN; ++c)
        if (c * MP_SCAN < S) {
#pragma unroll
            for (int j = c ? 0 : 1; j < MP_SCAN; ++j) s += bx >= tb.item0[c * MP_SCAN + j] ? 1 : 0;
        }
    const int b = s / Hkv;
    const int h = s - b * Hkv;
    const int cu0 = tb.cu_q[b];
    const int n_b = tb.cu_q[b + 1] - cu0;
    const int old = tb.len[s] + tb.off[b];                  // keys of the segment before this call
    const int kc = (old + chunk - 1) / chunk;               // key ranges of every group of this segment
    const int idx = bx - tb.item0[s];
    const int grp = idx / (kc + 1);
    const int part = idx - grp * (kc + 1);
    const bool tri = part == kc;                            // the run's own new rows
    const int R = n_b * G;                                  // query rows of the run per KV head
    const int ntiles = (R + TILE_RT - 1) / TILE_RT;
    if (n_b <= 0) return;                                   // (never taken: a cache without positions owns no item)

    const int64_t seg = tb.start[s];
    char* kseg = reinterpret_cast<char*>(tb.k[b]) + seg * C::ROW_BYTES;
    char* vseg = reinterpret_cast<char*>(tb.v[b]) + seg * C::ROW_BYTES;
    const char* kn_base = reinterpret_cast<const char*>(k_new + h * kn_h + (int64_t)cu0 * kn_p);
    const char* vn_base = reinterpret_cast<const char*>(v_new + h * vn_h + (int64_t)cu0 * vn_p);

    // ---- the append: rows old .. old + n_b - 1 of the segment, by ONE item per segment (nobody reads them in this launch) ----
    if (tri && grp == 0) {
        const int chunks = n_b * C::CPR;
        for (int e = threadIdx.x; e < 2 * chunks; e += MP_THREADS) {
            const bool is_v = e >= chunks;
            const int c = e - (is_v ? chunks : 0);
            const int p = c / C::CPR, cc = c % C::CPR;
            const char* src = (is_v ? vn_base + (int64_t)p * vn_p * 2 : kn_base + (int64_t)p * kn_p * 2) + cc * 16;
            char* dst = (is_v ? vseg : kseg) + (int64_t)(old + p) * C::ROW_BYTES + cc * 16;
            *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
        }
    }

    // ---- this wave's row tile ----
    const int tile = grp * MP_WAVES + wave;
    if (tile >= ntiles) return;                             // (wave-uniform; the kernel has no barrier)
    const int r_l = tile * TILE_RT + l15;                     // this lane's query row (a column of S^T and O^T)
    const bool rvalid = r_l < R;
    const int p_l = rvalid ? r_l / G : 0;
    const int g_l = r_l - p_l * G;
    const int r_last = min(tile * TILE_RT + TILE_RT - 1, R - 1);
    // the keys the wave visits, [k0, kend) of its source, and the keys this lane's row sees of them (key < limit)
    const int k0 = tri ? 0 : part * chunk;
    const int kend = tri ? r_last / G + 1 : min(old, k0 + chunk);      // (> k0: a key range is never empty)
    const int limit = rvalid ? (tri ? p_l + 1 : kend) : 0;
    const char* kb = tri ? kn_base : kseg;
    const char* vb = tri ? vn_base : vseg;
    const int64_t krow = tri ? kn_p * 2 : (int64_t)C::ROW_BYTES;       // bytes between two keys
    const int64_t vrow = tri ? vn_p * 2 : (int64_t)C::ROW_BYTES;

    __shared__ __attribute__((aligned(16))) char lds[MP_WAVES * C::WAVE_LDS];
    char* wl = lds + wave * C::WAVE_LDS;

    // rows past the wave's last key are clamped to it (always a row that exists) and masked below
    auto load_k = [&](u32x4 (&kr)[2][C::KK], int t0) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            int key = t0 + sub * 16 + l15;
            key = key < kend ? key : kend - 1;
            const char* kp = kb + (int64_t)key * krow + quad * 16;
#pragma unroll
            for (int kk = 0; kk < C::KK; ++kk) kr[sub][kk] = *reinterpret_cast<const u32x4*>(kp + kk * 64);
        }
    };
    auto load_v = [&](u32x4 (&vr)[C::VLOADS], int t0) {
#pragma unroll
        for (int it = 0; it < C::VLOADS; ++it) {
            const int c = it * WAVE + lane;
            int key = t0 + c / C::CPR;
            key = key < kend ? key : kend - 1;
            vr[it] = *reinterpret_cast<const u32x4*>(vb + (int64_t)key * vrow + (c % C::CPR) * 16);
        }
    };
#include "kvz_prefill_walk.inc"

    // ---- the row's partial (m, l, a[D]) to the item's slot ----
    float lr = l_run;
    lr += __shfl_xor(lr, 16, 64);
    lr += __shfl_xor(lr, 32, 64);
    if (!rvalid) return;
    const int64_t slot = (int64_t)bx * MP_GROUP + wave * TILE_RT + l15;
    float* po = part_o + slot * D + quad * 4;
#pragma unroll
    for (int db = 0; db < C::DB; ++db) *reinterpret_cast<f4*>(po + db * 16) = o[db];
    if (quad == 0) *reinterpret_cast<float2*>(part_ml + slot * 2) = make_float2(m_run, lr);
}

// merge, per (head, packed position, group member), the partials of the row's (segment, group): kc key ranges and the triangle.
// grid = (T, Hkv); block = 128 threads = (512 / D) rows x D / 4 column quads, looping over the G rows of the position.
constexpr int CB_THREADS = 128;
template <typename T, int D>
__global__ __launch_bounds__(CB_THREADS) void multi_prefill_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                                         Table tb, int B, int Hkv, int G, int Ttot, int chunk,
                                                                         T* __restrict__ out) {
    typedef typename Half<T>::v4 v4;
    constexpr int C4 = D / 4;
    constexpr int ROWS = CB_THREADS / C4;
    const int i = blockIdx.x, h = blockIdx.y;
    int b = 0;             // the last cache whose first position is not beyond i (caches without positions share the next one's)
#pragma unroll
    for (int j = 1; j < MP_MAXB; ++j) b += (j < B && i >= tb.cu_q[j]) ? 1 : 0;
    const int s = b * Hkv + h;
    const int p = i - tb.cu_q[b];
    const int old = tb.len[s] + tb.off[b];
    const int per = (old + chunk - 1) / chunk + 1;          // partials of a row: the key ranges and the triangle
    const int first = tb.item0[s];
    const int c4 = threadIdx.x % C4;
    for (int g = threadIdx.x / C4; g < G; g += ROWS) {
        const int r = p * G + g;
        const int grp = r / MP_GROUP;
        const int64_t slot0 = ((int64_t)first + (int64_t)grp * per) * MP_GROUP + (r - grp * MP_GROUP);
        float M = -INFINITY;
        for (int j = 0; j < per; ++j) M = fmaxf(M, part_ml[(slot0 + (int64_t)j * MP_GROUP) * 2]);
        f4 acc = f4{0.f, 0.f, 0.f, 0.f};
        float l = 0.f;
#pragma unroll 4
        for (int j = 0; j < per; ++j) {
            const int64_t sl = slot0 + (int64_t)j * MP_GROUP;
            const float2 ml = *reinterpret_cast<const float2*>(part_ml + sl * 2);
            const f4 a = *reinterpret_cast<const f4*>(part_o + sl * D + c4 * 4);
            const float w = (ml.x == -INFINITY) ? 0.f : exp2f(ml.x - M);
            acc[0] += w * a[0]; acc[1] += w * a[1]; acc[2] += w * a[2]; acc[3] += w * a[3];
            l += w * ml.y;
        }
        v4 z;
#pragma unroll
        for (int e = 0; e < 4; ++e) z[e] = (T)((l > 0.f) ? acc[e] / l : 0.f);
        *reinterpret_cast<u32x2*>(out + (((int64_t)h * Ttot + i) * G + g) * D + c4 * 4) = __builtin_bit_cast(u32x2, z);
    }
}

struct Ws { float* part_ml; float* part_o; size_t items; size_t bytes; };
static inline Ws workspace(void* ws, int T, int B, int Hkv, int G, int D) {
    const size_t rg = (size_t)Hkv * ((size_t)T * G / MP_GROUP + B);   // >= the (segment, group) pairs of any packing of T positions
    Ws w;
    w.items = (size_t)target_items(B * Hkv) + 2 * rg;
    char* p = reinterpret_cast<char*>(ws);
    w.part_ml = reinterpret_cast<float*>(p);
    p += align256(w.items * MP_GROUP * 2 * sizeof(float));
    w.part_o = reinterpret_cast<float*>(p);
    p += align256(w.items * MP_GROUP * D * sizeof(float));
    w.bytes = (size_t)(p - reinterpret_cast<char*>(ws));
    return w;
}

template <typename T, int D>
static int launch(const void* q, int64_t qs_head, int64_t qs_group, int64_t qs_pos, const Table& tb, int items, int chunk,
                  const void* k_new, const void* v_new, int64_t kn_h, int64_t kn_p, int64_t vn_h, int64_t vn_p, int B, int Hkv, int G,
                  int Ttot, float scale, void* out, const Ws& w, hipStream_t stream) {
    ProfScope ps("multi_prefill", stream);
    hipLaunchKernelGGL((multi_prefill_split_kernel<T, D>), dim3(items), dim3(MP_THREADS), 0, stream, reinterpret_cast<const T*>(q),
                       qs_head, qs_group, qs_pos, tb, reinterpret_cast<const T*>(k_new), reinterpret_cast<const T*>(v_new), kn_h, kn_p,
                       vn_h, vn_p, B * Hkv, Hkv, G, chunk, scale, w.part_o, w.part_ml);
    KVZ_CHECK_LAUNCH("multi_prefill_split_kernel");
    hipLaunchKernelGGL((multi_prefill_combine_kernel<T, D>), dim3(Ttot, Hkv), dim3(CB_THREADS), 0, stream, w.part_o, w.part_ml, tb, B,
                       Hkv, G, Ttot, chunk, reinterpret_cast<T*>(out));
    KVZ_CHECK_LAUNCH("multi_prefill_combine_kernel");
    return KVZ_OK;
}

}  // namespace mprefill
}  // namespace kvz

using namespace kvz;

extern "C" size_t kvz_multi_prefill_workspace_bytes(int T, int B, int Hkv, int G, int D) {
    if (T <= 0 || B <= 0 || Hkv <= 0 || G <= 0 || D <= 0) return 0;
    return mprefill::workspace(nullptr, T, B, Hkv, G, D).bytes;
}

extern "C" int kvz_multi_prefill(const void* q, int64_t q_stride_head, int64_t q_stride_group, int64_t q_stride_pos,
                                 const int32_t* cu_q_host, void* const* k_ptrs_host, void* const* v_ptrs_host,
                                 const int32_t* seg_start_host, const int32_t* len_host, const int32_t* slack_host,
                                 const int32_t* offset_host, const void* k_new, const void* v_new, int64_t k_new_head_stride,
                                 int64_t k_new_pos_stride, int64_t v_new_head_stride, int64_t v_new_pos_stride, int B, int Hkv, int G,
                                 int D, float scale, int dtype, void* out, void* ws, size_t ws_bytes, kvz_stream_t stream_) {
    using namespace kvz::mprefill;
    hipStream_t stream = (hipStream_t)stream_;
    KVZ_REQUIRE(q && cu_q_host && k_ptrs_host && v_ptrs_host && seg_start_host && len_host && slack_host && offset_host && k_new && v_new
                    && out, KVZ_EINVAL, "kvz_multi_prefill: null pointer");
    KVZ_REQUIRE(B > 0 && Hkv > 0 && G > 0, KVZ_EINVAL, "kvz_multi_prefill: bad shape (B %d, Hkv %d, G %d)", B, Hkv, G);
    KVZ_REQUIRE(D == 64 || D == 128, KVZ_EUNSUPPORTED, "kvz_multi_prefill: head_dim %d unsupported (64 or 128)", D);
    KVZ_REQUIRE(B <= MP_MAXB && Hkv <= MP_MAXH && (int64_t)B * Hkv <= MP_MAXS && G <= MP_MAXG, KVZ_EUNSUPPORTED,
                "kvz_multi_prefill: %d caches x %d KV heads x %d query heads per KV head unsupported (B <= %d, Hkv <= %d, "
                "B*Hkv <= %d segments, G <= %d)", B, Hkv, G, MP_MAXB, MP_MAXH, MP_MAXS, MP_MAXG);
    KVZ_REQUIRE(dtype == KVZ_F16 || dtype == KVZ_BF16, KVZ_EINVAL, "kvz_multi_prefill: bad dtype %d", dtype);
    KVZ_REQUIRE(aligned16(q) && aligned16(k_new) && aligned16(v_new) && aligned16(out) && aligned16(ws), KVZ_EINVAL,
                "kvz_multi_prefill: pointers must be 16-byte aligned");
    KVZ_REQUIRE(q_stride_head % 8 == 0 && q_stride_group % 8 == 0 && q_stride_pos % 8 == 0, KVZ_EINVAL,
                "kvz_multi_prefill: the strides of q must be multiples of 8 elements");
    KVZ_REQUIRE(k_new_head_stride % 8 == 0 && k_new_pos_stride % 8 == 0 && v_new_head_stride % 8 == 0 && v_new_pos_stride % 8 == 0,
                KVZ_EINVAL, "kvz_multi_prefill: the strides of the new rows must be multiples of 8 elements");
    KVZ_REQUIRE(cu_q_host[0] == 0, KVZ_EINVAL, "kvz_multi_prefill: cu_q[0] = %d, must be 0", cu_q_host[0]);
    const int S = B * Hkv;
    Table tb = {};
    int64_t weighted = 0;                  // sum over the (segment, group) pairs of the segment's old length: what the key ranges are cut from
    for (int b = 0; b < B; ++b) {
        const int64_t n = (int64_t)cu_q_host[b + 1] - cu_q_host[b];
        KVZ_REQUIRE(n >= 0, KVZ_EINVAL, "kvz_multi_prefill: cu_q decreases at cache %d (%d -> %d)", b, cu_q_host[b], cu_q_host[b + 1]);
        tb.cu_q[b] = cu_q_host[b];
        if (n == 0) continue;              // takes no part: nothing of it is looked at
        const int off = offset_host[b];
        KVZ_REQUIRE(k_ptrs_host[b] && v_ptrs_host[b], KVZ_EINVAL, "kvz_multi_prefill: null K or V pointer of cache %d", b);
        KVZ_REQUIRE(aligned16(k_ptrs_host[b]) && aligned16(v_ptrs_host[b]), KVZ_EINVAL,
                    "kvz_multi_prefill: K and V of cache %d must be 16-byte aligned", b);
        KVZ_REQUIRE(off >= 0, KVZ_EINVAL, "kvz_multi_prefill: offset[%d] = %d is negative", b, off);
        KVZ_REQUIRE(off + n <= slack_host[b], KVZ_EINVAL,
                    "kvz_multi_prefill: cache %d: offset %d + %lld new rows do not fit in slack = %d: they would run into the next segment",
                    b, off, (long long)n, slack_host[b]);
        KVZ_REQUIRE(n * G < ((int64_t)1 << 30), KVZ_EUNSUPPORTED, "kvz_multi_prefill: too many packed query rows for one launch");
        tb.k[b] = k_ptrs_host[b];
        tb.v[b] = v_ptrs_host[b];
        tb.off[b] = off;
        const int groups = groups_of((int)n, G);
        for (int h = 0; h < Hkv; ++h) {
            const int s = b * Hkv + h;
            KVZ_REQUIRE(seg_start_host[s] >= 0 && len_host[s] >= 0 && (int64_t)seg_start_host[s] + len_host[s] + slack_host[b] <= INT_MAX,
                        KVZ_EINVAL, "kvz_multi_prefill: bad segment start %d or length %d of cache %d, head %d", seg_start_host[s],
                        len_host[s], b, h);
            tb.start[s] = seg_start_host[s];
            tb.len[s] = len_host[s];
            weighted += (int64_t)groups * ((int64_t)len_host[s] + off);
        }
    }
    const int Ttot = cu_q_host[B];
    for (int b = B; b <= MP_MAXB; ++b) tb.cu_q[b] = Ttot;
    if (Ttot == 0) return KVZ_OK;
    KVZ_REQUIRE(ws, KVZ_EINVAL, "kvz_multi_prefill: null pointer");
    const Ws w = workspace(ws, Ttot, B, Hkv, G, D);
    KVZ_REQUIRE(ws_bytes >= w.bytes, KVZ_EWORKSPACE, "kvz_multi_prefill: workspace too small (%zu bytes, %zu needed)", ws_bytes, w.bytes);
    // the key ranges: chunks of the weighted sum of the old lengths, a multiple of 128 keys
    const int target = target_items(S);
    const int64_t chunk64 = chunk_of(weighted, target);
    KVZ_REQUIRE(chunk64 <= INT_MAX - 128, KVZ_EINVAL, "kvz_multi_prefill: %lld keys in one call", (long long)weighted);
    const int chunk = (int)chunk64;
    int64_t items = 0;
    for (int s = 0; s <= MP_MAXS; ++s) {
        tb.item0[s] = s <= S ? (int32_t)items : INT_MAX;
        if (s >= S) continue;
        const int b = s / Hkv;
        const int n = tb.cu_q[b + 1] - tb.cu_q[b];
        if (n > 0) {
            const int old = tb.len[s] + tb.off[b];
            items += (int64_t)groups_of(n, G) * ((old + chunk - 1) / chunk + 1);
        }
        KVZ_REQUIRE(items < ((int64_t)1 << 31), KVZ_EUNSUPPORTED, "kvz_multi_prefill: too many packed query rows for one launch");
    }
    KVZ_REQUIRE((size_t)items <= w.items, KVZ_EWORKSPACE, "kvz_multi_prefill: %lld work items exceed the %zu the workspace holds",
                (long long)items, w.items);
#define KVZ_MP_ARGS q, q_stride_head, q_stride_group, q_stride_pos, tb, (int)items, chunk, k_new, v_new, k_new_head_stride, \
                    k_new_pos_stride, v_new_head_stride, v_new_pos_stride, B, Hkv, G, Ttot, scale, out, w, stream
#define KVZ_MP_CALL(T, DD) return launch<T, DD>(KVZ_MP_ARGS)
    KVZ_DISPATCH_HALF_D(dtype, D, KVZ_MP_CALL);
#undef KVZ_MP_CALL
#undef KVZ_MP_ARGS
}
