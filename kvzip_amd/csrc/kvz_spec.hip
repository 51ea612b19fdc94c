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
// The work of a block for one item is ONE function (spec_item of kvz_spec_step.h) instantiated for the two kinds of item, so that the
// shared items keep compile-time row strides and a scalar key limit; its tile step, key loop and merge are the text that
// fork_attn_kernel includes too (kvz_nt_step.inc, kvz_nt_merge.inc: DESIGN.md 3.12).  The header and the body of a block
// (kvz_spec_block.inc) are shared with the tree form of the step, kvz_tree.hip, whose attention kernel is a unit of
// its own so that the kernels here compile as they always did.
#include "kvz_spec_step.h"
#include "../../include/kvzip_hip_spec.h"

namespace kvz {
namespace spec {

template <typename T, int D, int NT>
__global__ __launch_bounds__(SP_THREADS) void spec_attn_kernel(
    const T* __restrict__ q, T* k, T* v, const int32_t* __restrict__ k_start, const int32_t* __restrict__ k_len, int k_len_offset,
    HeadMeta hm, int host_meta, const T* __restrict__ k_new, const T* __restrict__ v_new, int64_t kn_hstride, int64_t kn_pstride,
    int64_t vn_hstride, int64_t vn_pstride, int t, int Hkv, int G, int target_items, float scale, float* __restrict__ part_o,
    float* __restrict__ part_ml, int n_rtiles) {
#define KVZ_SPEC_TREE false
#define KVZ_SPEC_ANC nullptr
#include "kvz_spec_block.inc"
#undef KVZ_SPEC_TREE
#undef KVZ_SPEC_ANC
}

// merge, per (head, position, group row), the partials of the head's key ranges and of its triangle.  grid = (Hkv, t, G);
// block = 1024 threads = (1024/D) slices of the partials x D columns.  out = (T)(a / l).  This is combine_partials of kvz_combine.h
// spelled out: the other four combine kernels call it, this one exceeded the timing margin when it did and no cause was found
// (profiles/combine_shared_ab.txt).  A fix to the combine is made in both places.
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

template <typename T, int D>
static int launch_combine(const SpecPlan& p, const int32_t* k_len, int k_len_offset, int t, int Hkv, int G, void* out, hipStream_t stream) {
    hipLaunchKernelGGL((spec_combine_kernel<T, D>), dim3(Hkv, t, G), dim3(CB_THREADS), 0, stream, p.w.part_o, p.w.part_ml, k_len,
                       k_len_offset, p.hm, p.host, t, Hkv, G, p.target, p.n_rtiles, reinterpret_cast<T*>(out));
    KVZ_CHECK_LAUNCH("spec_combine_kernel");
    return KVZ_OK;
}

int spec_combine(const SpecPlan& p, const int32_t* k_len, int k_len_offset, int t, int Hkv, int G, int D, int dtype, void* out,
                 hipStream_t stream) {
#define KVZ_COMBINE_CALL(T, DD) return launch_combine<T, DD>(p, k_len, k_len_offset, t, Hkv, G, out, stream)
    KVZ_DISPATCH_HALF_D(dtype, D, KVZ_COMBINE_CALL);
#undef KVZ_COMBINE_CALL
}

template <typename T, int D>
static int launch_spec(const void* q, void* k, void* v, const int32_t* k_start, const int32_t* k_len, int k_len_offset,
                       const int32_t* meta_host, const void* k_new, const void* v_new, int64_t kn_h, int64_t kn_p, int64_t vn_h,
                       int64_t vn_p, int t, int Hkv, int G, float scale, int dtype, void* out, void* ws, hipStream_t stream) {
    const SpecPlan p = spec_plan(meta_host, t, Hkv, G, D, ws);
    ProfScope ps("spec_attn", stream);
#define KVZ_SPEC_LAUNCH(NT)                                                                                                              \
    hipLaunchKernelGGL((spec_attn_kernel<T, D, NT>), p.grid, dim3(SP_THREADS), 0, stream, reinterpret_cast<const T*>(q),                \
                       reinterpret_cast<T*>(k), reinterpret_cast<T*>(v), k_start, k_len, k_len_offset, p.hm, p.host,                    \
                       reinterpret_cast<const T*>(k_new), reinterpret_cast<const T*>(v_new), kn_h, kn_p, vn_h, vn_p, t, Hkv, G,         \
                       p.target, scale, p.w.part_o, p.w.part_ml, p.n_rtiles)
    if (p.nt == 2) KVZ_SPEC_LAUNCH(2);
    else KVZ_SPEC_LAUNCH(1);
#undef KVZ_SPEC_LAUNCH
    KVZ_CHECK_LAUNCH("spec_attn_kernel");
    return spec_combine(p, k_len, k_len_offset, t, Hkv, G, D, dtype, out, stream);
}

int spec_validate(const char* who, const void* q, const void* k_cache, const void* v_cache, const int32_t* k_start, const int32_t* k_len,
                  int k_len_offset, const int32_t* k_meta_host, int slack, const void* k_new, const void* v_new,
                  int64_t k_new_head_stride, int64_t k_new_pos_stride, int64_t v_new_head_stride, int64_t v_new_pos_stride, int t, int Hkv,
                  int G, int D, int dtype, const void* out, const void* ws) {
    KVZ_REQUIRE(q && k_cache && v_cache && k_new && v_new && out && ws, KVZ_EINVAL, "%s: null pointer", who);
    KVZ_REQUIRE((k_start && k_len) || k_meta_host, KVZ_EINVAL,
                "%s: no segment metadata (k_start and k_len on the device, or k_meta_host)", who);
    KVZ_REQUIRE(Hkv > 0 && G > 0, KVZ_EINVAL, "%s: bad shape (Hkv %d, G %d)", who, Hkv, G);
    KVZ_REQUIRE(t >= 1, KVZ_EINVAL, "%s: t = %d new positions (at least 1)", who, t);
    KVZ_REQUIRE(k_len_offset >= 0, KVZ_EINVAL, "%s: k_len_offset = %d is negative", who, k_len_offset);
    KVZ_REQUIRE(D == 64 || D == 128, KVZ_EUNSUPPORTED, "%s: head_dim %d unsupported (64 or 128)", who, D);
    KVZ_REQUIRE((int64_t)t * G <= SP_MAXROWS, KVZ_EUNSUPPORTED,
                "%s: %d positions x %d query heads per KV head unsupported (t*G <= %d query rows per head)", who, t, G,
                SP_MAXROWS);
    KVZ_REQUIRE(Hkv <= SP_MAXH, KVZ_EUNSUPPORTED, "%s: %d KV heads unsupported (Hkv <= %d)", who, Hkv, SP_MAXH);
    KVZ_REQUIRE(dtype == KVZ_F16 || dtype == KVZ_BF16, KVZ_EINVAL, "%s: bad dtype %d", who, dtype);
    KVZ_REQUIRE(aligned16(q) && aligned16(k_cache) && aligned16(v_cache) && aligned16(k_new) && aligned16(v_new) && aligned16(out)
                    && aligned16(ws), KVZ_EINVAL, "%s: pointers must be 16-byte aligned", who);
    KVZ_REQUIRE(k_new_head_stride % 8 == 0 && k_new_pos_stride % 8 == 0 && v_new_head_stride % 8 == 0 && v_new_pos_stride % 8 == 0,
                KVZ_EINVAL, "%s: the strides of the new rows must be multiples of 8 elements", who);
    KVZ_REQUIRE((int64_t)k_len_offset + t <= slack, KVZ_EINVAL,
                "%s: k_len_offset = %d plus t = %d exceeds slack = %d: the new rows do not fit behind the segments", who, k_len_offset, t,
                slack);
    if (k_meta_host)
        for (int h = 0; h < Hkv; ++h)
            KVZ_REQUIRE(k_meta_host[h] >= 0 && k_meta_host[Hkv + h] >= 0, KVZ_EINVAL, "%s: negative segment start or length of head %d",
                        who, h);
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
    const char* who = "kvz_spec_attn_append";
    const int rc = spec::spec_validate(who, q, k_cache, v_cache, k_start, k_len, k_len_offset, k_meta_host, slack, k_new, v_new,
                                       k_new_head_stride, k_new_pos_stride, v_new_head_stride, v_new_pos_stride, t, Hkv, G, D, dtype, out,
                                       ws);
    if (rc != KVZ_OK) return rc;
    KVZ_REQUIRE(ws_bytes >= kvz_spec_attn_workspace_bytes(t, Hkv, G, D), KVZ_EWORKSPACE, "%s: workspace too small (%zu bytes, %zu needed)",
                who, ws_bytes, kvz_spec_attn_workspace_bytes(t, Hkv, G, D));
#define KVZ_SPEC_ARGS q, k_cache, v_cache, k_start, k_len, k_len_offset, k_meta_host, k_new, v_new, k_new_head_stride, k_new_pos_stride, \
                      v_new_head_stride, v_new_pos_stride, t, Hkv, G, scale, dtype, out, ws, stream
#define KVZ_SPEC_CALL(T, DD) return spec::launch_spec<T, DD>(KVZ_SPEC_ARGS)
    KVZ_DISPATCH_HALF_D(dtype, D, KVZ_SPEC_CALL);
#undef KVZ_SPEC_CALL
#undef KVZ_SPEC_ARGS
}
