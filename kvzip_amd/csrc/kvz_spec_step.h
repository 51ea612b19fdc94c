// kvz_spec_step.h — what the two forms of the verify step share (kvz_spec.hip: a chain of t positions; kvz_tree.hip: a tree of t
// nodes): the work of a block for one item, the workspace and the work-item cut; the body of a block is kvz_spec_block.inc.  The two
// attention kernels live in translation units of their own and take the body of a block as text, so that the chain kernels come out
// of the compiler exactly as they did before the tree form existed (a second kernel over spec_item in the same unit, or a function
// boundary around the body, changes their register allocation and schedule); the combine kernel and the argument checks exist once,
// in kvz_spec.hip, and the tree form calls them through the two host functions declared at the end.
#ifndef KVZ_SPEC_STEP_H
#define KVZ_SPEC_STEP_H
#include "kvz_wave_tile.h"

#include <type_traits>

namespace kvz {
namespace spec {

constexpr int SP_THREADS = 512;
constexpr int SP_WAVES = 8;
constexpr int SP_MAXH = 64;
constexpr int SP_MAXROWS = 64;       // t*G

struct HeadMeta { int32_t start[SP_MAXH]; int32_t len[SP_MAXH]; };
// Tree form (kvzip_hip_tree.h): the t new positions are the nodes of a tree in topological order; bit j of m[p] says that new row j
// is visible to node p (bit p is set, no bit above p).  t <= 64 nodes: 512 bytes that travel by value like HeadMeta.
struct AncMasks { uint64_t m[SP_MAXROWS]; };

// The key loop and the merge of a block's waves for one item: keys c0 .. c1 of `len` rows at kbase / vbase (row strides kstr / vstr
// bytes), row tiles rt0 .. rt0 + NT - 1 of the R query rows of head h.  TRI: the item is a triangle (key j is visible to query row r iff
// j <= r / G; kstr / vstr are the position strides of k_new / v_new); otherwise every key below c1 is visible to every row.
// TREE (a triangle item of the tree form): key j is visible to query row r iff bit j of anc->m[r / G] is set.  A lane owns one query
// row per row tile, so it keeps that row's mask in two registers; the chain forms never touch `anc`.
template <typename T, int D, int NT, bool TRI, bool TREE = false>
__device__ __forceinline__ void spec_item(const T* __restrict__ q, const char* kbase, const char* vbase, const int64_t kstr,
                                          const int64_t vstr, const int len, const int c0, const int c1, const int h, const int R,
                                          const int G, const int rt0, const float scale, float* __restrict__ po,
                                          float* __restrict__ pml, const int64_t slot0, char* lds,
                                          const AncMasks* anc = nullptr) {
    static_assert(TRI || !TREE, "only the item over the new keys has a mask among them");
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
    uint64_t vis[TREE ? NT : 1];  // TREE: the new keys visible to this lane's query row, one bit each
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int r = (rt0 + i) * TILE_RT + l15;
        rows_valid[i] = max(0, min(TILE_RT, R - (rt0 + i) * TILE_RT));
        const bool qvalid = l15 < rows_valid[i];
        lim[i] = qvalid ? min(c1, r / G + 1) : 0;
        if constexpr (TREE) vis[i] = qvalid ? anc->m[r / G] : 0;  // (r < R = t * G: a node of the call)
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
                if constexpr (TREE) x = ((vis[i] >> (key & 63)) & 1) ? x : -INFINITY;  // (key < c1 <= t <= 64; no bit at or above c1)
                else x = key < limit ? x : -INFINITY;
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

// What one step launches: filled by spec_plan from the arguments of an entry point.
struct SpecPlan { HeadMeta hm; int host; int n_rtiles; int nt; int target; dim3 grid; SpecWs w; };
static inline SpecPlan spec_plan(const int32_t* meta_host, int t, int Hkv, int G, int D, void* ws) {
    SpecPlan p;
    p.n_rtiles = (t * G + TILE_RT - 1) / TILE_RT;
    p.w = spec_ws(ws, t, Hkv, G, D);
    p.host = meta_host != nullptr;
    for (int h = 0; h < SP_MAXH; ++h) {
        p.hm.start[h] = p.host && h < Hkv ? meta_host[h] : 0;
        p.hm.len[h] = p.host && h < Hkv ? meta_host[Hkv + h] : 0;
    }
    // two row tiles per block from two row tiles on; three or four row tiles are two blocks per work item (grid.y)
    p.nt = p.n_rtiles >= 2 ? 2 : 1;
    p.target = spec_items(Hkv);
    p.grid = dim3(Hkv + p.target + Hkv, (p.n_rtiles + p.nt - 1) / p.nt);
    return p;
}

// ---- defined in kvz_spec.hip ----
// The argument checks both forms share; `who` names the entry point in the messages.  KVZ_OK or the code to return.
int spec_validate(const char* who, const void* q, const void* k_cache, const void* v_cache, const int32_t* k_start, const int32_t* k_len,
                  int k_len_offset, const int32_t* k_meta_host, int slack, const void* k_new, const void* v_new,
                  int64_t k_new_head_stride, int64_t k_new_pos_stride, int64_t v_new_head_stride, int64_t v_new_pos_stride, int t, int Hkv,
                  int G, int D, int dtype, const void* out, const void* ws);
// The second launch of a step: spec_combine_kernel over the partials of plan p.
int spec_combine(const SpecPlan& p, const int32_t* k_len, int k_len_offset, int t, int Hkv, int G, int D, int dtype, void* out,
                 hipStream_t stream);

}  // namespace spec
}  // namespace kvz
#endif  // KVZ_SPEC_STEP_H
