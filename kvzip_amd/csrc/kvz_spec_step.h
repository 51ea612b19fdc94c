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
// (key < c1 <= t <= 64 in a triangle item of the tree form, and no bit of vis[] at or above c1)
#define KVZ_NT_VISIBLE(i, key) (TREE ? (bool)((vis[i] >> ((key) & 63)) & 1) : (key) < (TRI ? lim[i] : c1))
    constexpr int BLOCK_WAVES = SP_WAVES;
#include "kvz_nt_step.inc"

    constexpr int rt_first = 0;  // (slot0 is the slot of row tile rt0)
#include "kvz_nt_merge.inc"
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
