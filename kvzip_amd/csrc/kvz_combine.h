// kvz_combine.h - the second launch of the split-K decode-attention calls: one block merges the n partials of one query row.  The
// combine kernels of kvz_attn.hip, kvz_retain.hip, kvz_fork.hip and kvz_multi.hip keep their index math - which row, where its
// partials lie, where it goes - and call combine_partials for the rest.  A combine is a kernel of its own, so nothing
// here touches the key loop of a split kernel.  spec_combine_kernel (kvz_spec.hip, also the second launch of kvz_tree.hip) is the same
// body spelled out: it missed the timing margin as a caller (profiles/combine_shared_ab.txt); a fix here is made there too.
// Also here: the workspace carve that kvz_attn.hip and kvz_retain.hip share.
#pragma once
#include "kvz_wave_tile.h"

namespace kvz {

constexpr int CB_THREADS = 1024;    // (1024 / D) slices of the partials x D columns
constexpr int CB_PER = 8;           // partials per thread on the fast path

// where one partial lies: its (m, l) pair and its D floats
struct Partial { const float* ml; const float* o; };

// {first work item, number of items} of head h among Hkv heads of len_of(hh) keys: the cut of the split kernels (which spell it out in
// front of their key loops), for the combine kernels
struct ItemRange { int first_item; int nsp; };
template <typename LenOf>
__device__ __forceinline__ ItemRange item_range(LenOf len_of, int Hkv, int h, int target_items) {
    int total = 0;
    for (int hh = 0; hh < Hkv; ++hh) total += len_of(hh);
    const int chunk = chunk_of(total, target_items);
    int first_item = 0;
    for (int hh = 0; hh < h; ++hh) first_item += max(1, (len_of(hh) + chunk - 1) / chunk);
    return ItemRange{first_item, max(1, (len_of(h) + chunk - 1) / chunk)};
}

// out_row[0 .. D) = (T)(a / l) over the partials partial_of(0) .. partial_of(n - 1), n >= 1, weights exp2(m_s - max m); 0 where l = 0.
// Called by all CB_THREADS threads of the block.  Thread (slice, d) sums column d of the partials slice, slice + SLICES, ..., in that
// order, and the slice's share of the denominator with them; thread d then adds the slices in order.
template <typename T, int D, typename PartialOf>
__device__ __forceinline__ void combine_partials(int n, PartialOf partial_of, T* __restrict__ out_row) {
    constexpr int SLICES = CB_THREADS / D;
    const int tid = threadIdx.x;
    const int d = tid % D, slice = tid / D;

    __shared__ float s_red[CB_THREADS / WAVE];
    __shared__ float s_acc[SLICES][D];
    __shared__ float s_l[SLICES];

    float acc = 0.f, lp = 0.f;
    if (n <= CB_PER * SLICES) {
        // ONE round trip to memory: every thread issues the loads of its (up to 8) partials - statistics and its column - before
        // anything depends on them; the row maximum is then a block reduction over registers
        float2 ml[CB_PER];
        float ov[CB_PER];
#pragma unroll
        for (int i = 0; i < CB_PER; ++i) {
            const int s2 = slice + i * SLICES;
            const Partial p = partial_of(min(s2, n - 1));
            ml[i] = *reinterpret_cast<const float2*>(p.ml);
            ov[i] = p.o[d];
            if (s2 >= n) ml[i] = make_float2(-INFINITY, 0.f);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < CB_PER; ++i) mx = fmaxf(mx, ml[i].x);
        mx = wave_reduce_max(mx);
        if ((tid & 63) == 0) s_red[tid >> 6] = mx;
        __syncthreads();
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < CB_THREADS / WAVE; ++w) M = fmaxf(M, s_red[w]);
#pragma unroll
        for (int i = 0; i < CB_PER; ++i) {
            const float wgt = (ml[i].x == -INFINITY) ? 0.f : exp2f(ml[i].x - M);
            acc += wgt * ov[i];
            lp += wgt * ml[i].y;
        }
    } else {
        // more partials than the fast path holds in registers: the maximum first, then one pass over the partials
        float mx = -INFINITY;
        for (int s2 = tid; s2 < n; s2 += CB_THREADS) mx = fmaxf(mx, partial_of(s2).ml[0]);
        mx = wave_reduce_max(mx);
        if ((tid & 63) == 0) s_red[tid >> 6] = mx;
        __syncthreads();
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < CB_THREADS / WAVE; ++w) M = fmaxf(M, s_red[w]);
        for (int s2 = slice; s2 < n; s2 += SLICES) {
            const Partial p = partial_of(s2);
            const float2 ml = *reinterpret_cast<const float2*>(p.ml);
            const float wgt = (ml.x == -INFINITY) ? 0.f : exp2f(ml.x - M);
            acc += wgt * p.o[d];
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
        out_row[tid] = (T)((l > 0.f) ? a / l : 0.f);
    }
}

// ---- host: the workspace of kvz_varlen_attn and kvz_retain_attn (the same layout, byte for byte) ---------------------------------
// a reserved region (the per-(head, row tile) counters of the round-2 in-kernel merge; its size is part of the ABI), the statistics,
// the partial outputs
struct SplitWs { uint32_t* counters; float* part_ml; float* part_o; size_t bytes; };
static inline SplitWs split_ws(void* ws, int Hkv, int n_rtiles, int D) {
    const size_t items = (size_t)target_items(Hkv) + Hkv;
    SplitWs w;
    char* p = reinterpret_cast<char*>(ws);
    w.counters = reinterpret_cast<uint32_t*>(p);
    p += align256((size_t)Hkv * n_rtiles * sizeof(uint32_t));
    w.part_ml = reinterpret_cast<float*>(p);
    p += align256(items * n_rtiles * TILE_RT * 2 * sizeof(float));
    w.part_o = reinterpret_cast<float*>(p);
    p += align256(items * n_rtiles * TILE_RT * D * sizeof(float));
    w.bytes = (size_t)(p - reinterpret_cast<char*>(ws));
    return w;
}

}  // namespace kvz
