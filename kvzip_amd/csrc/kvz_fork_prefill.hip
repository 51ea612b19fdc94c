// kvz_fork_prefill.hip — the packed first step of a forked decode: everything that is PRIVATE to a branch, for the query tokens of all
// branches of a wave, in one launch (gfx950; ABI and semantics: include/kvzip_hip_prefill.h).
//
// No reference counterpart (batch is hard-wired to 1 there).  The queries of B branches lie back to back in one packed sequence of
// T = cu_q[B] positions; the unmasked attention over the SHARED segments is one kvz_flash_fwd call over all T positions.  This file:
//   fork_prefill_kernel  one block per (run of positions = branch b, KV head h, group of FP_WAVES 16-row tiles of the branch's
//                        n_b * G query rows, row = p * G + g).  A WAVE owns one row tile and walks all its keys alone, 32 at a time:
//                          keys j <  t_b  come from tail[b, h, j],
//                          keys j >= t_b  come from k_new / v_new[h, cu_q[b] + j - t_b]  - never from the tail, so no block waits for
//                                         another block's write (no inter-block waiting),
//                        up to the last key its rows may see (bottom-right causal inside the branch: row (p, g) sees keys
//                        j < t_b + p + 1; key tiles above the diagonal of the wave's rows are never visited, the tiles on it are masked
//                        per element).  Tile scheme of kvz_fork.hip: S^T = K.Q^T on v_mfma_f32_16x16x32 with the K fragments straight
//                        from memory, O^T += V^T.P^T with V through a padded per-wave LDS tile read back transposed; softmax state
//                        in fp32, in the exp2 domain.  No wave shares anything with another one: no barrier, no workspace.
//                        The block of row-tile group 0 of every (b, h) copies the n_b new rows to tail[b, h, t_b : t_b + n_b].
//                        Epilogue, per row: with x1 = lse_shared * log2(e), (m, l, a) the tail's running maximum, denominator and
//                        fp32 accumulator, M = max(x1, m), w1 = 2^(x1 - M), w2 = 2^(m - M):
//                            out = fp16/bf16((w1 * o_shared + w2 * a) / (w1 + w2 * l))
//                        which is kvz_attn_merge_lse's formula with the tail side kept in fp32 and unnormalised (its LSE is
//                        m + log2 l): one division, one cast.  lse_shared = -inf gives fp16/bf16(a / l), the 'div' form of the decode
//                        combines.  Every lane loads the o_shared elements it overwrites before it writes them: out may be o_shared.
#include "kvz_wave_tile.h"

#include "../../include/kvzip_hip_prefill.h"

namespace kvz {
namespace fprefill {

constexpr int FP_WAVES = 4;          // row tiles of one block (one wave each, one wave per SIMD)
constexpr int FP_THREADS = FP_WAVES * WAVE;
constexpr int FP_MAXB = 16;
constexpr int FP_MAXH = 64;
constexpr int FP_MAXG = 64;

// the packing, by value: positions, tail index, tail length and first block of every run of positions (= branch)
struct Table {
    int32_t cu_q[FP_MAXB + 1];
    int32_t tail_of[FP_MAXB];      // the run's branch in the tails
    int32_t tail_len[FP_MAXB];     // ... and the rows that tail holds before the call
    int32_t blk0[FP_MAXB + 1];
};

template <typename T, int D>
__global__ __launch_bounds__(FP_THREADS) void fork_prefill_kernel(
    const T* __restrict__ q, int64_t qs_head, int64_t qs_group, int64_t qs_pos, T* tail_k, T* tail_v, int tail_cap,
    const T* __restrict__ k_new, const T* __restrict__ v_new, int64_t kn_h, int64_t kn_p, int64_t vn_h, int64_t vn_p, const T* o_shared,
    const float* __restrict__ lse_shared, T* out, Table tb, int B, int Hkv, int G, int Ttot, float scale) {
    typedef TileCfg<D> C;
    typedef typename Half<T>::v8 v8;
    typedef typename Half<T>::v4 v4;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int l15 = lane & 15, quad = lane >> 4;

    // ---- this block's (branch, head, row-tile group): block-uniform scalar work ----
    int b = 0;
    while (b + 1 < B && (int)blockIdx.x >= tb.blk0[b + 1]) ++b;
    const int cu0 = tb.cu_q[b];
    const int n_b = tb.cu_q[b + 1] - cu0;
    const int t_b = tb.tail_len[b];
    const int R = n_b * G;                                  // query rows of the branch per KV head
    const int ntiles = (R + TILE_RT - 1) / TILE_RT;
    const int groups = (ntiles + FP_WAVES - 1) / FP_WAVES;
    const int idx = (int)blockIdx.x - tb.blk0[b];
    const int h = idx / groups;
    const int grp = idx - h * groups;
    if (n_b <= 0 || h >= Hkv) return;                       // (never taken: a branch without positions owns no block)

    const int64_t trow0 = ((int64_t)tb.tail_of[b] * Hkv + h) * tail_cap;
    const char* tk_base = reinterpret_cast<const char*>(tail_k) + trow0 * C::ROW_BYTES;
    const char* tv_base = reinterpret_cast<const char*>(tail_v) + trow0 * C::ROW_BYTES;
    const char* kn_base = reinterpret_cast<const char*>(k_new + h * kn_h + (int64_t)cu0 * kn_p);
    const char* vn_base = reinterpret_cast<const char*>(v_new + h * vn_h + (int64_t)cu0 * vn_p);
    const int64_t kn_row = kn_p * 2, vn_row = vn_p * 2;     // bytes between two positions

    // ---- the append: rows t_b .. t_b + n_b - 1 of tail[b, h], by the block of row-tile group 0 (nobody reads them in this launch) ----
    if (grp == 0) {
        const int chunks = n_b * C::CPR;
        for (int e = threadIdx.x; e < 2 * chunks; e += FP_THREADS) {
            const bool is_v = e >= chunks;
            const int c = e - (is_v ? chunks : 0);
            const int p = c / C::CPR, cc = c % C::CPR;
            const char* src = (is_v ? vn_base + p * vn_row : kn_base + p * kn_row) + cc * 16;
            char* dst = reinterpret_cast<char*>(is_v ? tail_v : tail_k) + (trow0 + t_b + p) * C::ROW_BYTES + cc * 16;
            *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
        }
    }

    // ---- this wave's row tile ----
    const int tile = grp * FP_WAVES + wave;
    if (tile >= ntiles) return;                             // (wave-uniform; the kernel has no barrier)
    const int r_l = tile * TILE_RT + l15;                     // this lane's query row (a column of S^T and O^T)
    const bool rvalid = r_l < R;
    const int p_l = rvalid ? r_l / G : 0;
    const int g_l = r_l - p_l * G;
    const int limit = rvalid ? t_b + p_l + 1 : 0;           // keys the row sees
    const int r_last = min(tile * TILE_RT + TILE_RT - 1, R - 1);
    const int kend = t_b + r_last / G + 1;                  // keys the wave visits: the limit of its last row (>= 1)

    __shared__ __attribute__((aligned(16))) char lds[FP_WAVES * C::WAVE_LDS];
    char* wl = lds + wave * C::WAVE_LDS;

    // rows past the wave's last key are clamped to it (always a row that exists) and masked below
    auto load_k = [&](u32x4 (&kr)[2][C::KK], int t0) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            int key = t0 + sub * 16 + l15;
            key = key < kend ? key : kend - 1;
            const char* kp = (key < t_b ? tk_base + (int64_t)key * C::ROW_BYTES : kn_base + (int64_t)(key - t_b) * kn_row) + quad * 16;
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
            const char* vp = key < t_b ? tv_base + (int64_t)key * C::ROW_BYTES : vn_base + (int64_t)(key - t_b) * vn_row;
            vr[it] = *reinterpret_cast<const u32x4*>(vp + (c % C::CPR) * 16);
        }
    };
    const int k0 = 0;                                       // first key of the walk
#include "kvz_prefill_walk.inc"

    // ---- epilogue: merge with the partial result over the shared segments, one division, one cast ----
    float lr = l_run;
    lr += __shfl_xor(lr, 16, 64);
    lr += __shfl_xor(lr, 32, 64);
    if (!rvalid) return;
    const int64_t orow = ((int64_t)h * Ttot + cu0) * G + r_l;   // row of [Hkv, T, G]: (position, group member) = row of the branch
    const float x1 = lse_shared[orow] * 1.44269504088896340736f;
    const float M = fmaxf(x1, m_run);                           // (m_run is finite: every row sees its own key)
    const float w1 = exp2f(x1 - M), w2 = exp2f(m_run - M);
    const float den = w1 + w2 * lr;
    const T* osp = o_shared + orow * D + quad * 4;
    T* op = out + orow * D + quad * 4;
    v4 sh[C::DB];
#pragma unroll
    for (int db = 0; db < C::DB; ++db) sh[db] = __builtin_bit_cast(v4, *reinterpret_cast<const u32x2*>(osp + db * 16));
#pragma unroll
    for (int db = 0; db < C::DB; ++db) {
        v4 z;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // (a weight of 0 must silence the shared side whatever it holds: rows without a key are not written by every kernel)
            const float xs = w1 > 0.f ? w1 * (float)sh[db][e] : 0.f;
            z[e] = (T)((xs + w2 * o[db][e]) / den);
        }
        *reinterpret_cast<u32x2*>(op + db * 16) = __builtin_bit_cast(u32x2, z);
    }
}

template <typename T, int D>
static int launch(const void* q, int64_t qs_head, int64_t qs_group, int64_t qs_pos, void* tail_k, void* tail_v, int tail_cap,
                  const void* k_new, const void* v_new, int64_t kn_h, int64_t kn_p, int64_t vn_h, int64_t vn_p, const void* o_shared,
                  const float* lse_shared, void* out, const Table& tb, int blocks, int B, int Hkv, int G, int Ttot, float scale,
                  hipStream_t stream) {
    ProfScope ps("fork_prefill", stream);
    hipLaunchKernelGGL((fork_prefill_kernel<T, D>), dim3(blocks), dim3(FP_THREADS), 0, stream, reinterpret_cast<const T*>(q), qs_head,
                       qs_group, qs_pos, reinterpret_cast<T*>(tail_k), reinterpret_cast<T*>(tail_v), tail_cap,
                       reinterpret_cast<const T*>(k_new), reinterpret_cast<const T*>(v_new), kn_h, kn_p, vn_h, vn_p,
                       reinterpret_cast<const T*>(o_shared), lse_shared, reinterpret_cast<T*>(out), tb, B, Hkv, G, Ttot, scale);
    KVZ_CHECK_LAUNCH("fork_prefill_kernel");
    return KVZ_OK;
}

}  // namespace fprefill
}  // namespace kvz

using namespace kvz;

extern "C" size_t kvz_fork_prefill_workspace_bytes(int T, int B, int Hkv, int G, int D) {
    (void)T; (void)B; (void)Hkv; (void)G; (void)D;
    return 0;   // a wave walks the whole tail of its rows: no partial results
}

extern "C" int kvz_fork_prefill_tail(const void* q, int64_t q_stride_head, int64_t q_stride_group, int64_t q_stride_pos,
                                     const int32_t* cu_q_host, void* tail_k, void* tail_v, int tail_cap, const int32_t* tail_len_host,
                                     const void* k_new, const void* v_new, int64_t k_new_head_stride, int64_t k_new_pos_stride,
                                     int64_t v_new_head_stride, int64_t v_new_pos_stride, const void* o_shared, const float* lse_shared,
                                     void* out, const int32_t* branch_host, int B, int Hkv, int G, int D, float scale, int dtype,
                                     void* ws, size_t ws_bytes, kvz_stream_t stream_) {
    (void)ws; (void)ws_bytes;
    hipStream_t stream = (hipStream_t)stream_;
    KVZ_REQUIRE(q && cu_q_host && tail_k && tail_v && tail_len_host && k_new && v_new && o_shared && lse_shared && out, KVZ_EINVAL,
                "kvz_fork_prefill_tail: null pointer");
    KVZ_REQUIRE(B > 0 && Hkv > 0 && G > 0 && tail_cap >= 0, KVZ_EINVAL, "kvz_fork_prefill_tail: bad shape");
    KVZ_REQUIRE(D == 64 || D == 128, KVZ_EUNSUPPORTED, "kvz_fork_prefill_tail: head_dim %d unsupported (64 or 128)", D);
    KVZ_REQUIRE(B <= fprefill::FP_MAXB, KVZ_EUNSUPPORTED, "kvz_fork_prefill_tail: %d branches unsupported (B <= %d)", B, fprefill::FP_MAXB);
    KVZ_REQUIRE(Hkv <= fprefill::FP_MAXH, KVZ_EUNSUPPORTED, "kvz_fork_prefill_tail: %d KV heads unsupported (Hkv <= %d)", Hkv,
                fprefill::FP_MAXH);
    KVZ_REQUIRE(G <= fprefill::FP_MAXG, KVZ_EUNSUPPORTED, "kvz_fork_prefill_tail: %d query heads per KV head unsupported (G <= %d)", G,
                fprefill::FP_MAXG);
    KVZ_REQUIRE(dtype == KVZ_F16 || dtype == KVZ_BF16, KVZ_EINVAL, "kvz_fork_prefill_tail: bad dtype %d", dtype);
    KVZ_REQUIRE(aligned16(q) && aligned16(tail_k) && aligned16(tail_v) && aligned16(k_new) && aligned16(v_new) && aligned16(o_shared)
                    && aligned16(out) && (reinterpret_cast<uintptr_t>(lse_shared) & 3u) == 0, KVZ_EINVAL,
                "kvz_fork_prefill_tail: pointers must be 16-byte aligned (lse_shared: 4-byte)");
    KVZ_REQUIRE(q_stride_head % 8 == 0 && q_stride_group % 8 == 0 && q_stride_pos % 8 == 0, KVZ_EINVAL,
                "kvz_fork_prefill_tail: the strides of q must be multiples of 8 elements");
    KVZ_REQUIRE(k_new_head_stride % 8 == 0 && k_new_pos_stride % 8 == 0 && v_new_head_stride % 8 == 0 && v_new_pos_stride % 8 == 0,
                KVZ_EINVAL, "kvz_fork_prefill_tail: the strides of the new rows must be multiples of 8 elements");
    KVZ_REQUIRE(cu_q_host[0] == 0, KVZ_EINVAL, "kvz_fork_prefill_tail: cu_q[0] = %d, must be 0", cu_q_host[0]);
    fprefill::Table tb = {};
    int64_t blocks = 0;
    uint32_t seen = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = (int64_t)cu_q_host[b + 1] - cu_q_host[b];
        KVZ_REQUIRE(n >= 0, KVZ_EINVAL, "kvz_fork_prefill_tail: cu_q decreases at branch %d (%d -> %d)", b, cu_q_host[b], cu_q_host[b + 1]);
        const int tbr = branch_host ? branch_host[b] : b;
        KVZ_REQUIRE(tbr >= 0 && tbr < B && !(seen >> tbr & 1u), KVZ_EINVAL,
                    "kvz_fork_prefill_tail: branch_host[%d] = %d: not a permutation of 0 .. %d", b, tbr, B - 1);
        seen |= 1u << tbr;
        const int t = tail_len_host[tbr];
        KVZ_REQUIRE(t >= 0, KVZ_EINVAL, "kvz_fork_prefill_tail: tail_len[%d] = %d is negative", tbr, t);
        KVZ_REQUIRE(n == 0 || t + n <= tail_cap, KVZ_EINVAL,
                    "kvz_fork_prefill_tail: branch %d: tail_len %d + %lld new rows do not fit in tail_cap = %d", tbr, t, (long long)n,
                    tail_cap);
        const int64_t tiles = (n * G + TILE_RT - 1) / TILE_RT;
        tb.cu_q[b] = cu_q_host[b];
        tb.tail_of[b] = tbr;
        tb.tail_len[b] = t;
        tb.blk0[b] = (int32_t)blocks;
        blocks += (tiles + fprefill::FP_WAVES - 1) / fprefill::FP_WAVES * Hkv;
        KVZ_REQUIRE(blocks < ((int64_t)1 << 31), KVZ_EUNSUPPORTED, "kvz_fork_prefill_tail: too many packed query rows for one launch");
    }
    const int Ttot = cu_q_host[B];
    for (int b = B; b <= fprefill::FP_MAXB; ++b) {
        tb.cu_q[b] = Ttot;
        tb.blk0[b] = (int32_t)blocks;
    }
    if (Ttot == 0) return KVZ_OK;
#define KVZ_FP_ARGS q, q_stride_head, q_stride_group, q_stride_pos, tail_k, tail_v, tail_cap, k_new, v_new, k_new_head_stride,         \
                    k_new_pos_stride, v_new_head_stride, v_new_pos_stride, o_shared, lse_shared, out, tb, (int)blocks, B, Hkv, G, Ttot, \
                    scale, stream
#define KVZ_FP_CALL(T, DD) return fprefill::launch<T, DD>(KVZ_FP_ARGS)
    KVZ_DISPATCH_HALF_D(dtype, D, KVZ_FP_CALL);
#undef KVZ_FP_CALL
#undef KVZ_FP_ARGS
}
