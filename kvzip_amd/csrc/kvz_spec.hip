// kvz_spec.hip — one VERIFY step of draft-and-verify decoding on a pruned slack-layout cache: t consecutive new positions of one
// sequence in two launches, gfx950.
//
// No reference counterpart: the reference decodes one token per forward pass.  The R = t*G query rows of a KV head (row = p*G + g)
// attend to the `old` rows the head segment holds, unmasked, and to the new rows 0 .. p.  One step:
//   spec_attn_kernel     grid.x = Hkv triangle items ++ the shared work items, cut from the SUM of the ragged head lengths exactly as
//                        fork_attn_kernel cuts them.  The R rows form ceil(R/16) row tiles; a block keeps the K fragments and the
//                        staged V tile of a 32-key wave tile and applies them to the NT row tiles it owns, so the kept rows come from
//                        HBM once per step up to 32 query rows and twice up to 64 (NT = 2: three or four row tiles are two blocks per
//                        item, grid.y = 2).  A triangle item (h, tile group) attends its row tiles over the t NEW keys, which it takes
//                        from k_new / v_new (strided views of the projection output), never from the rows this launch writes: no
//                        block waits for another block's write.  It masks per element (key j visible to position p iff j <= p).  The
//                        triangle block of tile group 0 also copies the t rows into the slack, 16 bytes per store.
//   spec_combine_kernel  per (head, position, group row): merges the partials of the head's key ranges and of the triangle.
//                        Final normalisation: out = fp16/bf16(a / l)  (the 'div' form of tests/attn_probes.py, like the decode combine
//                        of kvz_attn.hip).
// The steps of the wave tile are spelled out here as in every kernel on kvz_wave_tile.h; the body of a block is ONE
// function instantiated for the two kinds of item, so that the shared items keep compile-time row strides and a scalar key limit.
#include "kvz_wave_tile.h"
#include "../../include/kvzip_hip_spec.h"

#include <type_traits>

namespace kvz {
namespace spec {

constexpr int SP_THREADS = 512;
constexpr int SP_WAVES = 8;
constexpr int SP_MAXH = 64;
constexpr int SP_MAXROWS = 64;       // t*G

struct HeadMeta { int32_t start[SP_MAXH]; int32_t len[SP_MAXH]; };

// The key loop and the merge of a block's waves for one item: keys c0 .. c1 of `len` rows at kbase / vbase (row strides kstr / vstr
// bytes), row tiles rt0 .. rt0 + NT - 1 of the R query rows of head h.  TRI: the item is a triangle (key j is visible to query row r iff
// j <= r / G; kstr / vstr are the position strides of k_new / v_new); otherwise every key below c1 is visible to every row.
template <typename T, int D, int NT, bool TRI>
__device__ __forceinline__ void spec_item(const T* __restrict__ q, const char* kbase, const char* vbase, const int64_t kstr,
                                          const int64_t vstr, const int len, const int c0, const int c1, const int h, const int R,
                                          const int G, const int rt0, const float scale, float* __restrict__ po,
                                          float* __restrict__ pml, const int64_t slot0, char* lds) {
    typedef TileCfg<D> C;
    typedef typename Half<T>::v8 v8;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int l15 = lane & 15, quad = lane >> 4;
    char* wl = lds + wave * C::WAVE_LDS;
    const float sl2 = scale * LOG2E;  // work in the exp2 domain

    // ---- stationary Q fragments, one per row tile (B operand of S^T = K.Q^T): col = query row, k = head-dim slice ----
    v8 qf[NT][C::KK];
    int rows_valid[NT];
    int lim[NT];  // TRI: keys visible to this lane's query row (its position + 1)
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int r = (rt0 + i) * TILE_RT + l15;
        rows_valid[i] = max(0, min(TILE_RT, R - (rt0 + i) * TILE_RT));
        const bool qvalid = l15 < rows_valid[i];
        lim[i] = qvalid ? min(c1, r / G + 1) : 0;
        const T* qp = q + (qvalid ? ((int64_t)h * R + r) * D : 0) + quad * 8;
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
            const char* kp = kbase + (int64_t)key * kstr + quad * 16;
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
            vr[it] = *reinterpret_cast<const u32x4*>(vbase + (int64_t)key * vstr + (c % C::CPR) * 16);
        }
    };
    // Two row tiles at head dim 128 leave no registers for a second K and V buffer (kvz_fork.hip: 51 registers spilled with them): there
    // the next tile's V rows are requested into the SAME registers right after the current ones have gone to LDS, and its K rows right
    // after the S^T products have consumed the current ones.
    constexpr bool VLATE = NT * D > 128;
    u32x4 kraw[2][C::KK], vraw[C::VLOADS], knext[VLATE ? 1 : 2][C::KK], vnext[VLATE ? 1 : C::VLOADS];
    // one 32-key tile of this wave, applied to the NT row tiles
    auto compute_tile = [&](u32x4 (&kr)[2][C::KK], u32x4 (&vr)[C::VLOADS], int t0, int t_next, auto refill) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < C::VLOADS; ++it) {
            const int c = it * WAVE + lane;
            *reinterpret_cast<u32x4*>(wl + (c / C::CPR) * C::VSTRIDE + (c % C::CPR) * 16) = vr[it];
        }
        if constexpr (decltype(refill)::value) load_v(vr, t_next);
        f4 s[NT][2];
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                s[i][sub] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < C::KK; ++kk)
                    s[i][sub] = Half<T>::mfma(__builtin_bit_cast(v8, kr[sub][kk]), qf[i][kk], s[i][sub]);
            }
        if constexpr (decltype(refill)::value) load_k(kr, t_next);  // (the K fragments are spent: the next tile's take their registers)
        v8 pb[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            float sv[8];
            float tmax = -INFINITY;
            const int limit = TRI ? lim[i] : c1;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = t0 + (j >> 2) * 16 + quad * 4 + (j & 3);
                float x = s[i][j >> 2][j & 3] * sl2;
                x = key < limit ? x : -INFINITY;
                sv[j] = x;
                tmax = fmaxf(tmax, x);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float m_new = fmaxf(m_run[i], tmax);
            const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;
            const float alpha = exp2f(m_run[i] - m_safe);
            float psum = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = exp2f(sv[j] - m_safe);
                psum += p;
                pb[i][j] = (T)p;
            }
            l_run[i] = l_run[i] * alpha + psum;
            m_run[i] = m_new;
#pragma unroll
            for (int db = 0; db < C::DB; ++db) {
                o[i][db][0] *= alpha; o[i][db][1] *= alpha; o[i][db][2] *= alpha; o[i][db][3] *= alpha;
            }
        }
        const char* trp = wl + (quad * 4 + (l15 >> 2)) * C::VSTRIDE + (l15 & 3) * 8;
#pragma unroll
        for (int db = 0; db < C::DB; ++db) {
            s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(trp + db * 32));
            s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(trp + 16 * C::VSTRIDE + db * 32));
            s8 both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
            for (int i = 0; i < NT; ++i) o[i][db] = Half<T>::mfma(__builtin_bit_cast(v8, both), pb[i], o[i][db]);
        }
    };
    // The wave's tiles, one requested AHEAD of the one being computed; the steady-state loop issues the next tile's loads
    // UNCONDITIONALLY and the last tile is computed after the loop (the load structure of varlen_attn_split2_kernel).
    const int t_first = c0 + wave * TILE_KT;
    constexpr int T_STEP = SP_WAVES * TILE_KT;
    if (t_first < c1) {
        load_k(kraw, t_first);
        load_v(vraw, t_first);
        int t0 = t_first;
#pragma unroll 1
        for (; t0 + T_STEP < c1; t0 += T_STEP) {
            if constexpr (!VLATE) {
                load_k(knext, t0 + T_STEP);
                load_v(vnext, t0 + T_STEP);
            }
            compute_tile(kraw, vraw, t0, t0 + T_STEP, std::integral_constant<bool, VLATE>{});
            if constexpr (!VLATE) {
#pragma unroll
                for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                    for (int kk = 0; kk < C::KK; ++kk) kraw[sub][kk] = knext[sub][kk];
#pragma unroll
                for (int it = 0; it < C::VLOADS; ++it) vraw[it] = vnext[it];
            }
        }
        compute_tile(kraw, vraw, t0, 0, std::false_type{});
    }

    // ---- merge the 8 waves of the block through LDS, one row tile after the other (each wave stages in its own V tile) ----
    constexpr int WSTR = D + 4;                          // floats per staged row (bank-conflict-free, see kvz_attn.hip)
    static_assert((TILE_RT * WSTR + 2 * TILE_RT) * 4 <= C::WAVE_LDS, "the wave's V tile holds its merge staging");
    float* wo = reinterpret_cast<float*>(wl);            // [16 q][D + 4]
    float* wm = wo + TILE_RT * WSTR;                     // [16] m, [16] l
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        float lr = l_run[i];
        lr += __shfl_xor(lr, 16, 64);
        lr += __shfl_xor(lr, 32, 64);
        const int rv = rows_valid[i];
        if (l15 < rv) {
#pragma unroll
            for (int db = 0; db < C::DB; ++db) *reinterpret_cast<f4*>(wo + l15 * WSTR + db * 16 + quad * 4) = o[i][db];
            if (quad == 0) { wm[l15] = m_run[i]; wm[16 + l15] = lr; }
        }
        __syncthreads();
        const int64_t pbase = slot0 + (int64_t)i * TILE_RT;
        for (int e = threadIdx.x; e < rv * (D / 4); e += SP_THREADS) {
            const int qq = e / (D / 4), d = (e % (D / 4)) * 4;
            float mw[SP_WAVES], M = -INFINITY;
#pragma unroll
            for (int w = 0; w < SP_WAVES; ++w) {
                mw[w] = reinterpret_cast<const float*>(lds + w * C::WAVE_LDS)[TILE_RT * WSTR + qq];
                M = fmaxf(M, mw[w]);
            }
            f4 acc4 = f4{0.f, 0.f, 0.f, 0.f};
            float lsum = 0.f;
#pragma unroll
            for (int w = 0; w < SP_WAVES; ++w) {
                const float* pw = reinterpret_cast<const float*>(lds + w * C::WAVE_LDS);
                const float wgt = (mw[w] == -INFINITY) ? 0.f : exp2f(mw[w] - M);
                const f4 ov = *reinterpret_cast<const f4*>(pw + qq * WSTR + d);
                acc4[0] += wgt * ov[0]; acc4[1] += wgt * ov[1]; acc4[2] += wgt * ov[2]; acc4[3] += wgt * ov[3];
                lsum += wgt * pw[TILE_RT * WSTR + 16 + qq];
            }
            *reinterpret_cast<f4*>(po + (pbase + qq) * D + d) = acc4;
            if (d == 0) *reinterpret_cast<float2*>(pml + (pbase + qq) * 2) = make_float2(M, lsum);
        }
        __syncthreads();  // (the staging of this row tile has been read: the next one may overwrite it)
    }
}

// Partial rows of the workspace: item i, row tile rt -> (i * n_rtiles + rt) * 16 rows; items 0 .. Hkv - 1 are the triangles of the
// heads, the shared work items follow in head order.
template <typename T, int D, int NT>
__global__ __launch_bounds__(SP_THREADS) void spec_attn_kernel(
    const T* __restrict__ q, T* k, T* v, const int32_t* __restrict__ k_start, const int32_t* __restrict__ k_len, int k_len_offset,
    HeadMeta hm, int host_meta, const T* __restrict__ k_new, const T* __restrict__ v_new, int64_t kn_hstride, int64_t kn_pstride,
    int64_t vn_hstride, int64_t vn_pstride, int t, int Hkv, int G, int target_items, float scale, float* __restrict__ part_o,
    float* __restrict__ part_ml, int n_rtiles) {
    typedef TileCfg<D> C;
    __shared__ __attribute__((aligned(16))) char lds[SP_WAVES * C::WAVE_LDS];
    const int R = t * G;
    const int rt0 = (int)blockIdx.y * NT;
    if (rt0 >= n_rtiles) return;
    auto len_of = [&](int hh) -> int { return (host_meta ? hm.len[hh] : k_len[hh]) + k_len_offset; };

    if ((int)blockIdx.x < Hkv) {
        // ---- triangle item: the row tiles of this group over the t new keys, read from k_new / v_new ----
        const int h = blockIdx.x;
        const T* kn = k_new + h * kn_hstride;
        const T* vn = v_new + h * vn_hstride;
        if (blockIdx.y == 0) {
            // the t new rows of head h go behind its segment: the only bytes of the cache this launch writes, and nothing reads them
            constexpr int CH = D * 2 / 16;
            const int64_t row0 = (int64_t)(host_meta ? hm.start[h] : k_start[h]) + len_of(h);
            for (int e = threadIdx.x; e < 2 * t * CH; e += SP_THREADS) {
                const bool is_v = e >= t * CH;
                const int i = e - (is_v ? t * CH : 0);
                const int p = i / CH, c = i - p * CH;
                const T* src = (is_v ? vn + p * vn_pstride : kn + p * kn_pstride) + c * 8;
                T* dst = (is_v ? v : k) + (row0 + p) * D + c * 8;
                *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
            }
        }
        // (the last row of the group sees the most keys: later ones are masked for every row of this block)
        const int last_row = min(R, (rt0 + NT) * TILE_RT) - 1;
        const int c1 = last_row / G + 1;
        spec_item<T, D, NT, true>(q, reinterpret_cast<const char*>(kn), reinterpret_cast<const char*>(vn), kn_pstride * 2,
                                  vn_pstride * 2, t, 0, c1, h, R, G, rt0, scale, part_o, part_ml,
                                  ((int64_t)h * n_rtiles + rt0) * TILE_RT, lds);
        return;
    }

    // ---- shared work item (wave-uniform scalar work) ----
    int total = 0;
    for (int hh = 0; hh < Hkv; ++hh) total += len_of(hh);
    const int chunk = chunk_of(total, target_items);
    int split = 0, first_item = 0, h = -1;
    {
        int bx = (int)blockIdx.x - Hkv, items = 0;
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
    const int len = len_of(h);
    const int64_t seg = host_meta ? hm.start[h] : k_start[h];
    const int c0 = split * chunk;
    const int c1 = min(len, c0 + chunk);
    spec_item<T, D, NT, false>(q, reinterpret_cast<const char*>(k) + seg * C::ROW_BYTES, reinterpret_cast<const char*>(v) + seg * C::ROW_BYTES,
                               C::ROW_BYTES, C::ROW_BYTES, len, c0, c1, h, R, G, rt0, scale, part_o, part_ml,
                               ((int64_t)(Hkv + first_item + split) * n_rtiles + rt0) * TILE_RT, lds);
}

// merge, per (head, position, group row), the partials of the head's key ranges and of its triangle.  grid = (Hkv, t, G);
// block = 1024 threads = (1024/D) slices of the partials x D columns.  out = (T)(a / l).
constexpr int CB_THREADS = 1024;
template <typename T, int D>
__global__ __launch_bounds__(CB_THREADS) void spec_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                                 const int32_t* __restrict__ k_len, int k_len_offset, HeadMeta hm,
                                                                 int host_meta, int t, int Hkv, int G, int target_items, int n_rtiles,
                                                                 T* __restrict__ out) {
    constexpr int SLICES = CB_THREADS / D;
    const int h = blockIdx.x, p = blockIdx.y, g = blockIdx.z;
    const int tid = threadIdx.x;
    const int d = tid % D, slice = tid / D;
    const int r = p * G + g;
    const int64_t orow = ((int64_t)h * t * G + r) * D;
    auto len_of = [&](int hh) -> int { return (host_meta ? hm.len[hh] : k_len[hh]) + k_len_offset; };
    int total = 0;
    for (int hh = 0; hh < Hkv; ++hh) total += len_of(hh);
    const int chunk = chunk_of(total, target_items);
    int first_item = 0;
    for (int hh = 0; hh < h; ++hh) first_item += max(1, (len_of(hh) + chunk - 1) / chunk);
    const int nsp = max(1, (len_of(h) + chunk - 1) / chunk);
    const int64_t in_tile = (int64_t)(r / TILE_RT) * TILE_RT + r % TILE_RT;
    const int64_t istride = (int64_t)n_rtiles * TILE_RT;
    const int n = nsp + 1;  // the key ranges of the head, then its triangle (every row sees at least its own position)
    auto slot = [&](int s2) -> int64_t { return (s2 < nsp ? (int64_t)(Hkv + first_item + s2) : (int64_t)h) * istride + in_tile; };

    __shared__ float s_red[CB_THREADS / WAVE];
    __shared__ float s_acc[SLICES][D];
    __shared__ float s_l[SLICES];

    constexpr int PER = 8;  // partials per thread on the fast path
    float acc = 0.f, lp = 0.f;
    if (n <= PER * SLICES) {
        // ONE round trip to memory: every thread issues the loads of its (up to 8) partials before anything depends on them
        float2 ml[PER];
        float ov[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int s2 = slice + i * SLICES;
            const int64_t sc = slot(min(s2, n - 1));
            ml[i] = *reinterpret_cast<const float2*>(part_ml + sc * 2);
            ov[i] = part_o[sc * D + d];
            if (s2 >= n) ml[i] = make_float2(-INFINITY, 0.f);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < PER; ++i) mx = fmaxf(mx, ml[i].x);
        mx = wave_reduce_max(mx);
        if ((tid & 63) == 0) s_red[tid >> 6] = mx;
        __syncthreads();
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < CB_THREADS / WAVE; ++w) M = fmaxf(M, s_red[w]);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const float wgt = (ml[i].x == -INFINITY) ? 0.f : exp2f(ml[i].x - M);
            acc += wgt * ov[i];
            lp += wgt * ml[i].y;
        }
    } else {
        // more partials than the fast path holds in registers: the maximum first, then one pass over the partials
        float mx = -INFINITY;
        for (int s2 = tid; s2 < n; s2 += CB_THREADS) mx = fmaxf(mx, part_ml[slot(s2) * 2]);
        mx = wave_reduce_max(mx);
        if ((tid & 63) == 0) s_red[tid >> 6] = mx;
        __syncthreads();
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < CB_THREADS / WAVE; ++w) M = fmaxf(M, s_red[w]);
        for (int s2 = slice; s2 < n; s2 += SLICES) {
            const int64_t sc = slot(s2);
            const float2 ml = *reinterpret_cast<const float2*>(part_ml + sc * 2);
            const float wgt = (ml.x == -INFINITY) ? 0.f : exp2f(ml.x - M);
            acc += wgt * part_o[sc * D + d];
            lp += wgt * ml.y;
        }
    }
    s_acc[slice][d] = acc;
    if (d == 0) s_l[slice] = lp;  // (every column of a slice holds the same share of the denominator)
    __syncthreads();
    if (tid < D) {
        float a = 0.f, l = 0.f;
#pragma unroll
        for (int sl = 0; sl < SLICES; ++sl) { a += s_acc[sl][tid]; l += s_l[sl]; }
        out[orow + tid] = (T)((l > 0.f) ? a / l : 0.f);
    }
}

// work items of the shared part: the decode kernel's count (one block per CU) less the triangle items of the same launch, never below
// a quarter of the CUs or the knob itself when it is smaller (the floor rule of kvz_fork.hip: fork_items)
static inline int spec_items(int Hkv) {
    const int t = target_items(Hkv);
    const int floor_items = device_cus() / 4;
    return t - Hkv > floor_items ? t - Hkv : (t < floor_items ? t : floor_items);
}
struct SpecWs { float* part_ml; float* part_o; size_t bytes; };
static inline SpecWs spec_ws(void* ws, int t, int Hkv, int G, int D) {
    const int n_rtiles = (t * G + TILE_RT - 1) / TILE_RT;
    int items = tunable(TUNE_ATTN_ITEMS);
    if (items <= 0) items = device_cus();
    // (at most target + Hkv shared items: every head rounds its count up; and the Hkv triangles)
    const size_t slots = ((size_t)items + 2 * (size_t)Hkv) * n_rtiles * TILE_RT;
    SpecWs w;
    char* p = reinterpret_cast<char*>(ws);
    w.part_ml = reinterpret_cast<float*>(p);
    p += align256(slots * 2 * sizeof(float));
    w.part_o = reinterpret_cast<float*>(p);
    p += align256(slots * D * sizeof(float));
    w.bytes = (size_t)(p - reinterpret_cast<char*>(ws));
    return w;
}

template <typename T, int D, int NT>
static void launch_spec_nt(dim3 grid, hipStream_t stream, const void* q, void* k, void* v, const int32_t* k_start, const int32_t* k_len,
                           int k_len_offset, const HeadMeta& hm, int host, const void* k_new, const void* v_new, int64_t kn_h,
                           int64_t kn_p, int64_t vn_h, int64_t vn_p, int t, int Hkv, int G, int target, float scale, const SpecWs& w,
                           int n_rtiles) {
    hipLaunchKernelGGL((spec_attn_kernel<T, D, NT>), grid, dim3(SP_THREADS), 0, stream, reinterpret_cast<const T*>(q),
                       reinterpret_cast<T*>(k), reinterpret_cast<T*>(v), k_start, k_len, k_len_offset, hm, host,
                       reinterpret_cast<const T*>(k_new), reinterpret_cast<const T*>(v_new), kn_h, kn_p, vn_h, vn_p, t, Hkv, G, target,
                       scale, w.part_o, w.part_ml, n_rtiles);
}

template <typename T, int D>
static int launch_spec(const void* q, void* k, void* v, const int32_t* k_start, const int32_t* k_len, int k_len_offset,
                       const int32_t* meta_host, const void* k_new, const void* v_new, int64_t kn_h, int64_t kn_p, int64_t vn_h,
                       int64_t vn_p, int t, int Hkv, int G, float scale, void* out, void* ws, hipStream_t stream) {
    const int n_rtiles = (t * G + TILE_RT - 1) / TILE_RT;
    const SpecWs w = spec_ws(ws, t, Hkv, G, D);
    HeadMeta hm;
    const int host = meta_host != nullptr;
    for (int h = 0; h < SP_MAXH; ++h) {
        hm.start[h] = host && h < Hkv ? meta_host[h] : 0;
        hm.len[h] = host && h < Hkv ? meta_host[Hkv + h] : 0;
    }
    ProfScope ps("spec_attn", stream);
    // two row tiles per block from two row tiles on; three or four row tiles are two blocks per work item (grid.y)
    const int nt = n_rtiles >= 2 ? 2 : 1;
    const int target = spec_items(Hkv);
    const dim3 grid(Hkv + target + Hkv, (n_rtiles + nt - 1) / nt);
    if (nt == 2)
        launch_spec_nt<T, D, 2>(grid, stream, q, k, v, k_start, k_len, k_len_offset, hm, host, k_new, v_new, kn_h, kn_p, vn_h, vn_p, t,
                                Hkv, G, target, scale, w, n_rtiles);
    else
        launch_spec_nt<T, D, 1>(grid, stream, q, k, v, k_start, k_len, k_len_offset, hm, host, k_new, v_new, kn_h, kn_p, vn_h, vn_p, t,
                                Hkv, G, target, scale, w, n_rtiles);
    KVZ_CHECK_LAUNCH("spec_attn_kernel");
    hipLaunchKernelGGL((spec_combine_kernel<T, D>), dim3(Hkv, t, G), dim3(CB_THREADS), 0, stream, w.part_o, w.part_ml, k_len,
                       k_len_offset, hm, host, t, Hkv, G, target, n_rtiles, reinterpret_cast<T*>(out));
    KVZ_CHECK_LAUNCH("spec_combine_kernel");
    return KVZ_OK;
}

}  // namespace spec
}  // namespace kvz

using namespace kvz;

extern "C" size_t kvz_spec_attn_workspace_bytes(int t, int Hkv, int G, int D) {
    if (t <= 0 || Hkv <= 0 || G <= 0 || D <= 0) return 0;
    return spec::spec_ws(nullptr, t, Hkv, G, D).bytes;
}

extern "C" int kvz_spec_attn_append(const void* q, void* k_cache, void* v_cache, const int32_t* k_start, const int32_t* k_len,
                                    int k_len_offset, const int32_t* k_meta_host, int slack, const void* k_new, const void* v_new,
                                    int64_t k_new_head_stride, int64_t k_new_pos_stride, int64_t v_new_head_stride,
                                    int64_t v_new_pos_stride, int t, int Hkv, int G, int D, float scale, int dtype, void* out, void* ws,
                                    size_t ws_bytes, kvz_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KVZ_REQUIRE(q && k_cache && v_cache && k_new && v_new && out && ws, KVZ_EINVAL, "kvz_spec_attn_append: null pointer");
    KVZ_REQUIRE((k_start && k_len) || k_meta_host, KVZ_EINVAL,
                "kvz_spec_attn_append: no segment metadata (k_start and k_len on the device, or k_meta_host)");
    KVZ_REQUIRE(Hkv > 0 && G > 0, KVZ_EINVAL, "kvz_spec_attn_append: bad shape (Hkv %d, G %d)", Hkv, G);
    KVZ_REQUIRE(t >= 1, KVZ_EINVAL, "kvz_spec_attn_append: t = %d new positions (at least 1)", t);
    KVZ_REQUIRE(k_len_offset >= 0, KVZ_EINVAL, "kvz_spec_attn_append: k_len_offset = %d is negative", k_len_offset);
    KVZ_REQUIRE(D == 64 || D == 128, KVZ_EUNSUPPORTED, "kvz_spec_attn_append: head_dim %d unsupported (64 or 128)", D);
    KVZ_REQUIRE((int64_t)t * G <= spec::SP_MAXROWS, KVZ_EUNSUPPORTED,
                "kvz_spec_attn_append: %d positions x %d query heads per KV head unsupported (t*G <= %d query rows per head)", t, G,
                spec::SP_MAXROWS);
    KVZ_REQUIRE(Hkv <= spec::SP_MAXH, KVZ_EUNSUPPORTED, "kvz_spec_attn_append: %d KV heads unsupported (Hkv <= %d)", Hkv, spec::SP_MAXH);
    KVZ_REQUIRE(dtype == KVZ_F16 || dtype == KVZ_BF16, KVZ_EINVAL, "kvz_spec_attn_append: bad dtype %d", dtype);
    KVZ_REQUIRE(aligned16(q) && aligned16(k_cache) && aligned16(v_cache) && aligned16(k_new) && aligned16(v_new) && aligned16(out)
                    && aligned16(ws), KVZ_EINVAL, "kvz_spec_attn_append: pointers must be 16-byte aligned");
    KVZ_REQUIRE(k_new_head_stride % 8 == 0 && k_new_pos_stride % 8 == 0 && v_new_head_stride % 8 == 0 && v_new_pos_stride % 8 == 0,
                KVZ_EINVAL, "kvz_spec_attn_append: the strides of the new rows must be multiples of 8 elements");
    KVZ_REQUIRE((int64_t)k_len_offset + t <= slack, KVZ_EINVAL,
                "kvz_spec_attn_append: k_len_offset = %d plus t = %d exceeds slack = %d: the new rows do not fit behind the segments",
                k_len_offset, t, slack);
    if (k_meta_host)
        for (int h = 0; h < Hkv; ++h)
            KVZ_REQUIRE(k_meta_host[h] >= 0 && k_meta_host[Hkv + h] >= 0, KVZ_EINVAL,
                        "kvz_spec_attn_append: negative segment start or length of head %d", h);
    KVZ_REQUIRE(ws_bytes >= kvz_spec_attn_workspace_bytes(t, Hkv, G, D), KVZ_EWORKSPACE,
                "kvz_spec_attn_append: workspace too small (%zu bytes, %zu needed)", ws_bytes, kvz_spec_attn_workspace_bytes(t, Hkv, G, D));
#define KVZ_SPEC_ARGS q, k_cache, v_cache, k_start, k_len, k_len_offset, k_meta_host, k_new, v_new, k_new_head_stride, k_new_pos_stride, \
                      v_new_head_stride, v_new_pos_stride, t, Hkv, G, scale, out, ws, stream
#define KVZ_SPEC_CALL(T, DD) return spec::launch_spec<T, DD>(KVZ_SPEC_ARGS)
    KVZ_DISPATCH_HALF_D(dtype, D, KVZ_SPEC_CALL);
#undef KVZ_SPEC_CALL
#undef KVZ_SPEC_ARGS
}
