// kvz_fork_branch.hip — move branch-private tail rows between the branch slots of a forked decode, all layers in one launch (gfx950).
//
// No reference counterpart (batch is 1 there).  A beam search over a fork (kvz_fork.hip) continues beam b from beam p's state at every
// step: the rows of slot p's tail - [B, Hkv, cap, D] per layer, K and V - have to be in slot b before the next decode step.  Every
// (layer, pair, head, K or V) is ONE contiguous run of rows * D * elem bytes at the start of a (slot, head) stripe, so the kernel is
// the copy loop of compact_gather_kernel (kvz_compact.hip) without a row list: 16-byte non-temporal loads and stores, BC_UNROLL of them
// in flight per lane.
//   grid.x  pieces of BC_THREADS * BC_UNROLL 16-byte vectors (16 KB) of a run - sized for the longest run of the call, a block
//           beyond the end of its own run leaves at once
//   grid.y  (pair, head, K or V)
//   grid.z  layer
// The copy is in place.  The host has checked that no slot is both a source and a destination and that no destination is named twice
// (one source may feed several destinations: its rows are read by several blocks and written by none), so no block reads what another
// one writes - no ordering between blocks, no second buffer, "no block waits for another block's write" holds trivially.
// Tables: the host knows every address, so the per-layer pointers and capacities and the pair list travel BY VALUE as kernel arguments
// (20 bytes per layer, 12 per pair: 2.8 KB of the 4 KB there are at 128 layers) - no device table, no upload, nothing to keep in step
// with the fork.  Models with more than 128 layers take one further launch per 128.
#include "kvz_common.h"
#include "../../include/kvzip_hip_branch.h"

namespace kvz {
namespace branch {

constexpr int BC_THREADS = 256;
constexpr int BC_UNROLL = 4;          // 16-byte moves in flight per lane
constexpr int BC_MAXL = 128;          // layers of one launch
constexpr int BC_MAXB = 16;           // branch slots (a pair list is shorter: sources and destinations are disjoint)
constexpr int BC_MAXH = 64;           // KV heads

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Table {
    void* k[BC_MAXL];                 // [B, Hkv, cap[l], D] tails of layer l
    void* v[BC_MAXL];
    int32_t cap[BC_MAXL];
    int32_t src[BC_MAXB];
    int32_t dst[BC_MAXB];
    int32_t rows[BC_MAXB];
};
static_assert(sizeof(Table) + 64 <= 4096, "the tables travel as kernel arguments");

__global__ __launch_bounds__(BC_THREADS) void fork_branch_copy_kernel(Table tb, int Hkv, int row_bytes) {
    const int layer = blockIdx.z;
    int y = blockIdx.y;               // ((pair * Hkv) + head) * 2 + (0: K, 1: V)
    const int is_v = y & 1;
    y >>= 1;
    const int pair = y / Hkv;
    const int h = y - pair * Hkv;
    const int64_t n16 = (int64_t)tb.rows[pair] * (row_bytes >> 4);            // 16-byte vectors of this run (rows <= cap: host-checked)
    const int64_t i0 = (int64_t)blockIdx.x * (BC_THREADS * BC_UNROLL) + threadIdx.x;
    if ((int64_t)blockIdx.x * (BC_THREADS * BC_UNROLL) >= n16) return;
    const int64_t stripe = (int64_t)tb.cap[layer] * row_bytes;                // bytes of one (slot, head)
    char* base = reinterpret_cast<char*>(is_v ? tb.v[layer] : tb.k[layer]);
    const u32x4* src = reinterpret_cast<const u32x4*>(base + ((int64_t)tb.src[pair] * Hkv + h) * stripe);
    u32x4* dst = reinterpret_cast<u32x4*>(base + ((int64_t)tb.dst[pair] * Hkv + h) * stripe);
    u32x4 r[BC_UNROLL];
#pragma unroll
    for (int u = 0; u < BC_UNROLL; ++u) {
        const int64_t i = i0 + u * BC_THREADS;
        // streamed once by this kernel: non-temporal, the shared rows of the next decode step are what L2 / MALL should keep
        if (i < n16) r[u] = __builtin_nontemporal_load(src + i);
    }
#pragma unroll
    for (int u = 0; u < BC_UNROLL; ++u) {
        const int64_t i = i0 + u * BC_THREADS;
        if (i < n16) __builtin_nontemporal_store(r[u], dst + i);
    }
}

}  // namespace branch
}  // namespace kvz

using namespace kvz;

extern "C" int kvz_fork_branch_copy(void* const* tail_k_host, void* const* tail_v_host, const int32_t* tail_cap_host, int n_layers,
                                    int B, int Hkv, int D, int elem_size, const int32_t* src_host, const int32_t* dst_host,
                                    const int32_t* rows_host, int n_pairs, kvz_stream_t stream_) {
    using namespace kvz::branch;
    hipStream_t stream = (hipStream_t)stream_;
    KVZ_REQUIRE(tail_k_host && tail_v_host && tail_cap_host, KVZ_EINVAL, "kvz_fork_branch_copy: null pointer");
    KVZ_REQUIRE(n_pairs == 0 || (src_host && dst_host && rows_host), KVZ_EINVAL, "kvz_fork_branch_copy: null pointer");
    KVZ_REQUIRE(n_layers > 0 && B > 0 && Hkv > 0 && D > 0 && elem_size > 0 && n_pairs >= 0, KVZ_EINVAL,
                "kvz_fork_branch_copy: bad shape (layers %d, B %d, Hkv %d, D %d, elem_size %d, pairs %d)", n_layers, B, Hkv, D, elem_size,
                n_pairs);
    const int64_t rb64 = (int64_t)D * elem_size;
    KVZ_REQUIRE(rb64 % 16 == 0 && rb64 <= (1 << 20), KVZ_EUNSUPPORTED,
                "kvz_fork_branch_copy: D * elem_size = %lld bytes per row is not a multiple of 16", (long long)rb64);
    KVZ_REQUIRE(B <= BC_MAXB && Hkv <= BC_MAXH, KVZ_EUNSUPPORTED,
                "kvz_fork_branch_copy: %d branch slots x %d KV heads unsupported (B <= %d, Hkv <= %d)", B, Hkv, BC_MAXB, BC_MAXH);
    const int row_bytes = (int)rb64;
    int min_cap = INT32_MAX;
    for (int l = 0; l < n_layers; ++l) {
        KVZ_REQUIRE(tail_k_host[l] && tail_v_host[l], KVZ_EINVAL, "kvz_fork_branch_copy: null K or V tail of layer %d", l);
        KVZ_REQUIRE(aligned16(tail_k_host[l]) && aligned16(tail_v_host[l]), KVZ_EINVAL,
                    "kvz_fork_branch_copy: the tails of layer %d must be 16-byte aligned", l);
        KVZ_REQUIRE(tail_cap_host[l] > 0, KVZ_EINVAL, "kvz_fork_branch_copy: tail capacity %d of layer %d", tail_cap_host[l], l);
        if (tail_cap_host[l] < min_cap) min_cap = tail_cap_host[l];
    }
    // the pair list: slots in range, sources and destinations disjoint, every destination once (B <= 16: one bit per slot)
    uint32_t src_set = 0, dst_set = 0;
    int max_rows = 0;
    for (int i = 0; i < n_pairs; ++i) {
        const int s = src_host[i], d = dst_host[i], r = rows_host[i];
        KVZ_REQUIRE(s >= 0 && s < B && d >= 0 && d < B, KVZ_EINVAL, "kvz_fork_branch_copy: pair %d (%d -> %d) names a slot outside [0, %d)",
                    i, s, d, B);
        KVZ_REQUIRE(s != d, KVZ_EINVAL, "kvz_fork_branch_copy: pair %d copies slot %d onto itself", i, s);
        KVZ_REQUIRE(!(dst_set & (1u << d)), KVZ_EINVAL, "kvz_fork_branch_copy: slot %d is a destination twice (pair %d)", d, i);
        src_set |= 1u << s;
        dst_set |= 1u << d;
        KVZ_REQUIRE(!(src_set & dst_set), KVZ_EINVAL,
                    "kvz_fork_branch_copy: a slot is both a source and a destination (pair %d: %d -> %d): the copy is in place", i, s, d);
        KVZ_REQUIRE(r >= 0, KVZ_EINVAL, "kvz_fork_branch_copy: rows[%d] = %d", i, r);
        KVZ_REQUIRE(r <= min_cap, KVZ_EINVAL, "kvz_fork_branch_copy: rows[%d] = %d exceed the smallest tail capacity %d", i, r, min_cap);
        if (r > max_rows) max_rows = r;
    }
    if (n_pairs == 0 || max_rows == 0) return KVZ_OK;   // nothing to move: nothing is launched
    // (disjoint sets with every destination once: at most B - 1 pairs, they fit the table)
    Table tb;
    for (int i = 0; i < BC_MAXB; ++i) {
        tb.src[i] = i < n_pairs ? src_host[i] : 0;
        tb.dst[i] = i < n_pairs ? dst_host[i] : 0;
        tb.rows[i] = i < n_pairs ? rows_host[i] : 0;
    }
    const int64_t n16 = (int64_t)max_rows * (row_bytes / 16);
    const int64_t per_block = BC_THREADS * BC_UNROLL;
    const int64_t gx = (n16 + per_block - 1) / per_block;
    KVZ_REQUIRE(gx <= INT32_MAX, KVZ_EINVAL, "kvz_fork_branch_copy: %d rows of %d bytes in one run", max_rows, row_bytes);
    ProfScope ps("fork_branch_copy", stream);
    for (int l0 = 0; l0 < n_layers; l0 += BC_MAXL) {
        const int nl = n_layers - l0 < BC_MAXL ? n_layers - l0 : BC_MAXL;
        for (int l = 0; l < BC_MAXL; ++l) {
            tb.k[l] = l < nl ? tail_k_host[l0 + l] : nullptr;
            tb.v[l] = l < nl ? tail_v_host[l0 + l] : nullptr;
            tb.cap[l] = l < nl ? tail_cap_host[l0 + l] : 0;
        }
        hipLaunchKernelGGL(fork_branch_copy_kernel, dim3((unsigned)gx, (unsigned)(n_pairs * Hkv * 2), (unsigned)nl), dim3(BC_THREADS), 0,
                           stream, tb, Hkv, row_bytes);
        KVZ_CHECK_LAUNCH("fork_branch_copy_kernel");
    }
    return KVZ_OK;
}
