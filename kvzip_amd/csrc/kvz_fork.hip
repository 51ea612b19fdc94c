// kvz_fork.hip — forked decode: B concurrent queries (branches) over ONE shared pruned KV cache, gfx950.
//
// No reference counterpart: the reference decodes one query at a time (batch is hard-wired to 1), so B answers
// read every kept K and V row B times.  Here every branch owns a small private TAIL ([B, Hkv, tail_cap, D]: the K,V of its query
// tokens and of the tokens it generates) and all branches share the flat cache read-only.  One decode step:
//   fork_attn_kernel     grid.x = B*Hkv tail items ++ the shared work items, cut from the SUM of the ragged head lengths exactly as
//                        varlen_attn_split2_kernel cuts them.  The R = B*G query rows of a head (row = b*G + g) form ceil(R/16) row
//                        tiles; a block keeps the K fragments and the staged V tile of a 32-key wave tile and applies them to the
//                        NT row tiles it owns (Q fragments, softmax state and accumulators per row tile in registers), so the shared
//                        rows come from HBM once per step whatever B is (NT = 2: four row tiles are two blocks, grid.y = 2 - the 256
//                        registers a lane of an 8-wave block has do not hold four sets of accumulators).  A tail item (b, h) first
//                        writes the branch's new K,V row to tail[b, h, tail_len[b]] (only this block reads that row; block-scope
//                        barrier before the read) and attends the G rows of (b, h) over tail rows 0 .. tail_len[b].
//   fork_combine_kernel  per (branch, head, group row): merges the partials of the head's key ranges and of the branch's tail.
//                        Final normalisation: out = fp16/bf16(a / l)  (the 'div' form of tests/attn_probes.py, as in every
//                        caller of kvz_combine.h); rows of an inactive branch (tail_len[b] < 0) are zero.
// No causal mask on the shared part: the whole context precedes every query.  The shared cache is never written.
//
// attn_merge_lse_kernel: merges two partial attention results by their natural-log LSEs (a branch's first step: kvz_flash_fwd over the
// shared segments, causal = 0, and over the branch's tail, causal = 1):
//   m = max(lse1, lse2);  w_i = exp(lse_i - m);  out = fp16/bf16((w1*o1 + w2*o2) / (w1 + w2));  both -inf -> 0.
#include "kvz_combine.h"

#include <type_traits>

namespace kvz {
namespace fork {

constexpr int FK_THREADS = 512;
constexpr int FK_WAVES = 8;
constexpr int FK_MAXH = 64;
constexpr int FK_MAXB = 16;
constexpr int FK_MAXROWS = 64;       // B*G

struct HeadMeta { int32_t start[FK_MAXH]; int32_t len[FK_MAXH]; };
struct TailLens { int32_t n[FK_MAXB]; };

template <typename T, int D, int NT>
__global__ __launch_bounds__(FK_THREADS) void fork_attn_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const int32_t* __restrict__ k_start,
    const int32_t* __restrict__ k_len, int k_len_offset, HeadMeta hm, int host_meta, T* tail_k, T* tail_v, int tail_cap, TailLens tl,
    const T* __restrict__ k_new, const T* __restrict__ v_new, int64_t kn_bstride, int64_t kn_hstride, int64_t vn_bstride,
    int64_t vn_hstride, int B, int Hkv, int G, int target_items, float scale, float* __restrict__ part_o,
    float* __restrict__ part_ml, float* __restrict__ tail_o, float* __restrict__ tail_ml, int n_rtiles) {
    typedef TileCfg<D> C;
    typedef typename Half<T>::v8 v8;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int l15 = lane & 15, quad = lane >> 4;
    const int R = B * G;
    const int GT = (G + TILE_RT - 1) / TILE_RT;   // row tiles of ONE branch (tail items)
    const int TG = (GT + NT - 1) / NT;        // blocks of one tail item: one unless a single branch has more than 16 * NT rows
    const int n_tail = B * Hkv * TG;

    // ---- this block's work item (wave-uniform scalar work) ----
    int h, len, c0, c1, branch = -1, grp = 0;
    int64_t slot0;                 // first partial row of row tile 0 of this item (+ 16 per row tile)
    const char *kbase, *vbase;
    float *po, *pml;
    if ((int)blockIdx.x < n_tail) {
        if (blockIdx.y != 0) return;
        grp = blockIdx.x % TG;
        branch = (blockIdx.x / TG) / Hkv;
        h = blockIdx.x / TG - branch * Hkv;
        const int t = tl.n[branch];
        if (t < 0) return;         // inactive branch: nothing written, the combine emits zeros
        const int64_t row0 = ((int64_t)branch * Hkv + h) * tail_cap;
        constexpr int CH = D * 2 / 16;
        // the branch's new row: only this block reads it (G > 16 * NT, one branch: each of the item's blocks writes the same bytes and
        // reads its own copy behind its own barrier)
        if ((int)threadIdx.x < 2 * CH) {
            const bool is_v = (int)threadIdx.x >= CH;
            const int c = (int)threadIdx.x - (is_v ? CH : 0);
            const char* src = reinterpret_cast<const char*>(is_v ? v_new + branch * vn_bstride + h * vn_hstride
                                                                 : k_new + branch * kn_bstride + h * kn_hstride) + c * 16;
            char* dst = reinterpret_cast<char*>(is_v ? tail_v : tail_k) + (row0 + t) * (D * 2) + c * 16;
            *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
        }
        __syncthreads();  // (workgroup-scope release/acquire: the row is visible to the loads of this block below)
        kbase = reinterpret_cast<const char*>(tail_k) + row0 * C::ROW_BYTES;
        vbase = reinterpret_cast<const char*>(tail_v) + row0 * C::ROW_BYTES;
        len = t + 1; c0 = 0; c1 = len;
        slot0 = ((int64_t)branch * Hkv + h) * GT * TILE_RT;
        po = tail_o; pml = tail_ml;
    } else {
        auto len_of = [&](int hh) -> int { return (host_meta ? hm.len[hh] : k_len[hh]) + k_len_offset; };
        int total = 0;
        for (int hh = 0; hh < Hkv; ++hh) total += len_of(hh);
        const int chunk = chunk_of(total, target_items);
        int split = 0, first_item = 0;
        h = -1;
        {
            int bx = (int)blockIdx.x - n_tail, items = 0;
            for (int hh = 0; hh < Hkv; ++hh) {
                const int n = max(1, (len_of(hh) + chunk - 1) / chunk);  // (an empty head still gets one item: it writes zeros)
                if (h < 0) {
                    if (bx < n) { h = hh; split = bx; first_item = items; }
                    else bx -= n;
                }
                items += n;
            }
        }
        if (h < 0) return;  // beyond the last item
        if ((int)blockIdx.y * NT >= n_rtiles) return;
        len = len_of(h);
        const int64_t seg = host_meta ? hm.start[h] : k_start[h];
        c0 = split * chunk;
        c1 = min(len, c0 + chunk);
        kbase = reinterpret_cast<const char*>(k) + seg * C::ROW_BYTES;
        vbase = reinterpret_cast<const char*>(v) + seg * C::ROW_BYTES;
        slot0 = ((int64_t)(first_item + split) * n_rtiles + (int64_t)blockIdx.y * NT) * TILE_RT;
        po = part_o; pml = part_ml;
    }

    __shared__ __attribute__((aligned(16))) char lds[FK_WAVES * C::WAVE_LDS];
    char* wl = lds + wave * C::WAVE_LDS;
    const float sl2 = scale * LOG2E;  // work in the exp2 domain

    {
        // ---- stationary Q fragments, one per row tile (B operand of S^T = K.Q^T): col = query row, k = head-dim slice ----
        v8 qf[NT][C::KK];
        int rows_valid[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            int bq, gq, nrows;
            if (branch >= 0) {
                const int gt = grp * NT + i;
                bq = branch; gq = gt * TILE_RT + l15;
                nrows = G - gt * TILE_RT;
            } else {
                const int rt = (int)blockIdx.y * NT + i;
                const int r = rt * TILE_RT + l15;
                bq = r / G; gq = r - bq * G;
                nrows = R - rt * TILE_RT;
            }
            rows_valid[i] = max(0, min(TILE_RT, nrows));
            const bool qvalid = l15 < rows_valid[i];
            const T* qp = q + (qvalid ? (((int64_t)bq * Hkv + h) * G + gq) * D : 0) + quad * 8;
#pragma unroll
            for (int kk = 0; kk < C::KK; ++kk) {
                u32x4 raw = *reinterpret_cast<const u32x4*>(qp + kk * 32);
                if (!qvalid) raw = u32x4{0, 0, 0, 0};
                qf[i][kk] = __builtin_bit_cast(v8, raw);
            }
        }
        float m_run[NT], l_run[NT];
        f4 o[NT][C::DB];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            m_run[i] = -INFINITY; l_run[i] = 0.f;
#pragma unroll
            for (int db = 0; db < C::DB; ++db) o[i][db] = f4{0.f, 0.f, 0.f, 0.f};
        }

        auto load_k = [&](u32x4 (&kr)[2][C::KK], int t0) {
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                int key = t0 + sub * 16 + l15;
                key = key < len ? key : len - 1;  // clamp (masked below)
                const char* kp = kbase + (int64_t)key * C::ROW_BYTES + quad * 16;
#pragma unroll
                for (int kk = 0; kk < C::KK; ++kk) kr[sub][kk] = *reinterpret_cast<const u32x4*>(kp + kk * 64);
            }
        };
        auto load_v = [&](u32x4 (&vr)[C::VLOADS], int t0) {
#pragma unroll
            for (int it = 0; it < C::VLOADS; ++it) {
                const int c = it * WAVE + lane;
                int key = t0 + c / C::CPR;
                key = key < len ? key : len - 1;
                vr[it] = *reinterpret_cast<const u32x4*>(vbase + (int64_t)key * C::ROW_BYTES + (c % C::CPR) * 16);
            }
        };
        constexpr int BLOCK_WAVES = FK_WAVES;
#define KVZ_NT_VISIBLE(i, key) ((key) < c1)  // (no causal mask: the whole context precedes every query)
#include "kvz_nt_step.inc"

        const int rt_first = grp * NT;  // (a tail item: slot0 is the slot of the branch's row tile 0; grp = 0 in a shared item)
#include "kvz_nt_merge.inc"
    }
}

// merge, per (head, branch, group row), the partials of the head's key ranges and of the branch's tail.  grid = (Hkv, B, G); the body
// is combine_partials of kvz_combine.h.
template <typename T, int D>
__global__ __launch_bounds__(CB_THREADS) void fork_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                                 const float* __restrict__ tail_o, const float* __restrict__ tail_ml,
                                                                 const int32_t* __restrict__ k_len, int k_len_offset, HeadMeta hm,
                                                                 int host_meta, TailLens tl, int B, int Hkv, int G, int target_items,
                                                                 int n_rtiles, T* __restrict__ out) {
    const int h = blockIdx.x, b = blockIdx.y, g = blockIdx.z;
    const int tid = threadIdx.x;
    const int64_t orow = (((int64_t)b * Hkv + h) * G + g) * D;
    if (tl.n[b] < 0) {  // inactive branch
        if (tid < D) out[orow + tid] = (T)0.f;
        return;
    }
    const ItemRange ir = item_range([&](int hh) -> int { return (host_meta ? hm.len[hh] : k_len[hh]) + k_len_offset; }, Hkv, h,
                                    target_items);
    const int nsp = ir.nsp;
    const int r = b * G + g;
    const int64_t base = ((int64_t)ir.first_item * n_rtiles + r / TILE_RT) * TILE_RT + r % TILE_RT;
    const int64_t istride = (int64_t)n_rtiles * TILE_RT;
    const int GT = (G + TILE_RT - 1) / TILE_RT;
    const int64_t trow = (((int64_t)b * Hkv + h) * GT + g / TILE_RT) * TILE_RT + g % TILE_RT;
    // the key ranges of the head, then the branch's tail (an active branch has at least its new row)
    combine_partials<T, D>(nsp + 1, [&](int s2) -> Partial {
        if (s2 >= nsp) return Partial{tail_ml + trow * 2, tail_o + trow * D};
        const int64_t pi = base + s2 * istride;
        return Partial{part_ml + pi * 2, part_o + pi * D};
    }, out + orow);
}

// out[r, :] = merge of (o1[r, :], lse1[r]) and (o2[r, :], lse2[r]); one thread per 8 elements (16 bytes)
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_merge_lse_kernel(const T* o1, const float* __restrict__ lse1, const T* o2,
                                                            const float* __restrict__ lse2, T* out, int64_t rows) {
    typedef typename Half<T>::v8 v8;
    constexpr int CPR = D / 8;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * CPR) return;
    const int64_t r = i / CPR;
    const float a = lse1[r], b = lse2[r];
    const float m = fmaxf(a, b);
    float w1 = 0.f, w2 = 0.f;
    if (m != -INFINITY) { w1 = expf(a - m); w2 = expf(b - m); }
    const float den = w1 + w2;
    const v8 x = *reinterpret_cast<const v8*>(o1 + i * 8);
    const v8 y = *reinterpret_cast<const v8*>(o2 + i * 8);
    v8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        // (a weight of 0 must silence its side whatever that side holds: rows without a key are not written by every kernel)
        const float xs = w1 > 0.f ? w1 * (float)x[j] : 0.f;
        const float ys = w2 > 0.f ? w2 * (float)y[j] : 0.f;
        z[j] = (T)(den > 0.f ? (xs + ys) / den : 0.f);
    }
    *reinterpret_cast<v8*>(out + i * 8) = z;
}

// work items of the shared part: the decode kernel's count (one block per CU) less the tail items of the same launch
static inline int fork_items(int B, int Hkv) {
    const int t = target_items(Hkv);
    const int floor_items = device_cus() / 4;
    return t - B * Hkv > floor_items ? t - B * Hkv : (t < floor_items ? t : floor_items);
}
struct ForkWs { float* part_ml; float* part_o; float* tail_ml; float* tail_o; size_t bytes; };
static inline ForkWs fork_ws(void* ws, int B, int Hkv, int G, int D) {
    const int n_rtiles = (B * G + TILE_RT - 1) / TILE_RT;
    const int GT = (G + TILE_RT - 1) / TILE_RT;
    // (sized for the largest item count any B gives: a workspace made once serves every wave of branches)
    int t = tunable(TUNE_ATTN_ITEMS);
    if (t <= 0) t = device_cus();
    const size_t items = (size_t)t + Hkv;
    const size_t trows = (size_t)B * Hkv * GT * TILE_RT;
    ForkWs w;
    char* p = reinterpret_cast<char*>(ws);
    w.part_ml = reinterpret_cast<float*>(p);
    p += align256(items * n_rtiles * TILE_RT * 2 * sizeof(float));
    w.part_o = reinterpret_cast<float*>(p);
    p += align256(items * n_rtiles * TILE_RT * D * sizeof(float));
    w.tail_ml = reinterpret_cast<float*>(p);
    p += align256(trows * 2 * sizeof(float));
    w.tail_o = reinterpret_cast<float*>(p);
    p += align256(trows * D * sizeof(float));
    w.bytes = (size_t)(p - reinterpret_cast<char*>(ws));
    return w;
}

template <typename T, int D, int NT>
static void launch_fork_nt(dim3 grid, hipStream_t stream, const void* q, const void* k, const void* v, const int32_t* k_start,
                           const int32_t* k_len, int k_len_offset, const HeadMeta& hm, int host, void* tail_k, void* tail_v, int tail_cap,
                           const TailLens& tl, const void* k_new, const void* v_new, int64_t kn_b, int64_t kn_h, int64_t vn_b, int64_t vn_h,
                           int B, int Hkv, int G, int target, float scale, const ForkWs& w, int n_rtiles) {
    hipLaunchKernelGGL((fork_attn_kernel<T, D, NT>), grid, dim3(FK_THREADS), 0, stream, reinterpret_cast<const T*>(q),
                       reinterpret_cast<const T*>(k), reinterpret_cast<const T*>(v), k_start, k_len, k_len_offset, hm, host,
                       reinterpret_cast<T*>(tail_k), reinterpret_cast<T*>(tail_v), tail_cap, tl, reinterpret_cast<const T*>(k_new),
                       reinterpret_cast<const T*>(v_new), kn_b, kn_h, vn_b, vn_h, B, Hkv, G, target, scale, w.part_o, w.part_ml, w.tail_o,
                       w.tail_ml, n_rtiles);
}

template <typename T, int D>
static int launch_fork(const void* q, const void* k, const void* v, const int32_t* k_start, const int32_t* k_len, int k_len_offset,
                       const int32_t* meta_host, void* tail_k, void* tail_v, int tail_cap, const int32_t* tail_len, const void* k_new,
                       const void* v_new, int64_t kn_b, int64_t kn_h, int64_t vn_b, int64_t vn_h, int B, int Hkv, int G, float scale,
                       void* out, void* ws, hipStream_t stream) {
    const int n_rtiles = (B * G + TILE_RT - 1) / TILE_RT;
    const ForkWs w = fork_ws(ws, B, Hkv, G, D);
    HeadMeta hm;
    const int host = meta_host != nullptr;
    for (int h = 0; h < FK_MAXH; ++h) {
        hm.start[h] = host && h < Hkv ? meta_host[h] : 0;
        hm.len[h] = host && h < Hkv ? meta_host[Hkv + h] : 0;
    }
    TailLens tl;
    for (int b = 0; b < FK_MAXB; ++b) tl.n[b] = b < B ? tail_len[b] : -1;
    ProfScope ps("fork_attn", stream);
    // two row tiles per block from two row tiles on; three or four row tiles are two blocks per work item (grid.y)
    const int nt = n_rtiles >= 2 ? 2 : 1;
    const int GT = (G + TILE_RT - 1) / TILE_RT, TG = (GT + nt - 1) / nt;
    const int target = fork_items(B * TG, Hkv);
    const dim3 grid(B * Hkv * TG + target + Hkv, (n_rtiles + nt - 1) / nt);
    if (nt == 2)
        launch_fork_nt<T, D, 2>(grid, stream, q, k, v, k_start, k_len, k_len_offset, hm, host, tail_k, tail_v, tail_cap, tl, k_new, v_new,
                                kn_b, kn_h, vn_b, vn_h, B, Hkv, G, target, scale, w, n_rtiles);
    else
        launch_fork_nt<T, D, 1>(grid, stream, q, k, v, k_start, k_len, k_len_offset, hm, host, tail_k, tail_v, tail_cap, tl, k_new, v_new,
                                kn_b, kn_h, vn_b, vn_h, B, Hkv, G, target, scale, w, n_rtiles);
    KVZ_CHECK_LAUNCH("fork_attn_kernel");
    hipLaunchKernelGGL((fork_combine_kernel<T, D>), dim3(Hkv, B, G), dim3(CB_THREADS), 0, stream, w.part_o, w.part_ml, w.tail_o,
                       w.tail_ml, k_len, k_len_offset, hm, host, tl, B, Hkv, G, target, n_rtiles, reinterpret_cast<T*>(out));
    KVZ_CHECK_LAUNCH("fork_combine_kernel");
    return KVZ_OK;
}

}  // namespace fork
}  // namespace kvz

using namespace kvz;

extern "C" size_t kvz_fork_attn_workspace_bytes(int B, int Hkv, int G, int D, int max_len_k) {
    if (B <= 0 || Hkv <= 0 || G <= 0 || D <= 0 || max_len_k < 0) return 0;
    return fork::fork_ws(nullptr, B, Hkv, G, D).bytes;
}

extern "C" int kvz_fork_attn_append(const void* q, const void* k_cache, const void* v_cache, const int32_t* k_start,
                                    const int32_t* k_len, int k_len_offset, const int32_t* k_meta_host, void* tail_k, void* tail_v,
                                    int tail_cap, const int32_t* tail_len_host, const void* k_new, const void* v_new,
                                    int64_t k_new_batch_stride, int64_t k_new_head_stride, int64_t v_new_batch_stride,
                                    int64_t v_new_head_stride, int B, int Hkv, int G, int D, float scale, int dtype, void* out, void* ws,
                                    size_t ws_bytes, kvz_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KVZ_REQUIRE(q && k_cache && v_cache && tail_k && tail_v && tail_len_host && k_new && v_new && out && ws
                    && ((k_start && k_len) || k_meta_host), KVZ_EINVAL, "kvz_fork_attn_append: null pointer");
    KVZ_REQUIRE(B > 0 && Hkv > 0 && G > 0 && tail_cap > 0 && k_len_offset >= 0, KVZ_EINVAL, "kvz_fork_attn_append: bad shape");
    KVZ_REQUIRE(D == 64 || D == 128, KVZ_EUNSUPPORTED, "kvz_fork_attn_append: head_dim %d unsupported (64 or 128)", D);
    KVZ_REQUIRE((int64_t)B * G <= fork::FK_MAXROWS && B <= fork::FK_MAXB, KVZ_EUNSUPPORTED,
                "kvz_fork_attn_append: %d branches x %d query heads per KV head unsupported (B*G <= %d query rows per head, B <= %d)", B, G,
                fork::FK_MAXROWS, fork::FK_MAXB);
    KVZ_REQUIRE(Hkv <= fork::FK_MAXH, KVZ_EUNSUPPORTED, "kvz_fork_attn_append: %d KV heads unsupported (<= %d)", Hkv, fork::FK_MAXH);
    KVZ_REQUIRE(dtype == KVZ_F16 || dtype == KVZ_BF16, KVZ_EINVAL, "kvz_fork_attn_append: bad dtype %d", dtype);
    KVZ_REQUIRE(aligned16(q) && aligned16(k_cache) && aligned16(v_cache) && aligned16(tail_k) && aligned16(tail_v) && aligned16(k_new)
                    && aligned16(v_new) && aligned16(out) && aligned16(ws), KVZ_EINVAL,
                "kvz_fork_attn_append: pointers must be 16-byte aligned");
    KVZ_REQUIRE(k_new_batch_stride % 8 == 0 && k_new_head_stride % 8 == 0 && v_new_batch_stride % 8 == 0 && v_new_head_stride % 8 == 0,
                KVZ_EINVAL, "kvz_fork_attn_append: the strides of the new rows must be multiples of 8 elements");
    for (int b = 0; b < B; ++b)
        KVZ_REQUIRE(tail_len_host[b] >= -1 && tail_len_host[b] < tail_cap, KVZ_EINVAL,
                    "kvz_fork_attn_append: tail_len[%d] = %d outside [-1, tail_cap = %d): the new row does not fit", b, tail_len_host[b],
                    tail_cap);
    if (k_meta_host)
        for (int h = 0; h < Hkv; ++h)
            KVZ_REQUIRE(k_meta_host[h] >= 0 && k_meta_host[Hkv + h] + k_len_offset >= 0, KVZ_EINVAL,
                        "kvz_fork_attn_append: negative segment start or length of head %d", h);
    KVZ_REQUIRE(ws_bytes >= kvz_fork_attn_workspace_bytes(B, Hkv, G, D, 0), KVZ_EWORKSPACE, "kvz_fork_attn_append: workspace too small");
#define KVZ_FORK_ARGS q, k_cache, v_cache, k_start, k_len, k_len_offset, k_meta_host, tail_k, tail_v, tail_cap, tail_len_host, k_new, v_new, \
                      k_new_batch_stride, k_new_head_stride, v_new_batch_stride, v_new_head_stride, B, Hkv, G, scale, out, ws, stream
#define KVZ_FORK_CALL(T, DD) return fork::launch_fork<T, DD>(KVZ_FORK_ARGS)
    KVZ_DISPATCH_HALF_D(dtype, D, KVZ_FORK_CALL);
#undef KVZ_FORK_CALL
#undef KVZ_FORK_ARGS
}

extern "C" int kvz_attn_merge_lse(const void* o1, const float* lse1, const void* o2, const float* lse2, void* out, int64_t rows, int D,
                                  int dtype, kvz_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KVZ_REQUIRE(o1 && lse1 && o2 && lse2 && out, KVZ_EINVAL, "kvz_attn_merge_lse: null pointer");
    KVZ_REQUIRE(rows >= 0 && rows < ((int64_t)1 << 40), KVZ_EINVAL, "kvz_attn_merge_lse: bad shape");
    KVZ_REQUIRE(D == 64 || D == 128, KVZ_EUNSUPPORTED, "kvz_attn_merge_lse: head_dim %d unsupported (64 or 128)", D);
    KVZ_REQUIRE(dtype == KVZ_F16 || dtype == KVZ_BF16, KVZ_EINVAL, "kvz_attn_merge_lse: bad dtype %d", dtype);
    KVZ_REQUIRE(aligned16(o1) && aligned16(o2) && aligned16(out), KVZ_EINVAL, "kvz_attn_merge_lse: pointers must be 16-byte aligned");
    if (rows == 0) return KVZ_OK;
    const int64_t n = rows * (D / 8);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
#define KVZ_MERGE_LAUNCH(T, DD)                                                                                                       \
    hipLaunchKernelGGL((fork::attn_merge_lse_kernel<T, DD>), grid, block, 0, stream, reinterpret_cast<const T*>(o1), lse1,              \
                       reinterpret_cast<const T*>(o2), lse2, reinterpret_cast<T*>(out), rows)
    KVZ_DISPATCH_HALF_D(dtype, D, KVZ_MERGE_LAUNCH);
#undef KVZ_MERGE_LAUNCH
    KVZ_CHECK_LAUNCH("attn_merge_lse_kernel");
    return KVZ_OK;
}
