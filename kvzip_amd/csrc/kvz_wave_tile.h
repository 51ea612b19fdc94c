// kvz_wave_tile.h - what the split-K attention kernels (kvz_attn.hip, kvz_fork.hip, kvz_multi.hip, kvz_fork_prefill.hip,
// kvz_multi_prefill.hip, kvz_spec.hip, kvz_retain.hip) share: the vector types, the MFMA traits, the constants of the wave tile and the host-side cut into work items.
//
// Tile scheme.  A WAVE owns a tile of 32 keys (KT) x 16 query rows (RT):
//   S^T = K.Q^T   on v_mfma_f32_16x16x32 with the K rows loaded straight from memory as the A operand (16 contiguous bytes per lane,
//                 no LDS) and the stationary Q fragment as the B operand: lane & 15 = one query row, lane >> 4 = a slice of the keys;
//   softmax       online, fp32, in the exp2 domain, state in registers;
//   O^T += V^T.P^T with the V rows staged through a padded per-wave LDS tile (VSTRIDE) and read back transposed by ds_read_b64_tr_b16.
// The steps of the tile themselves exist once per family of kernels, as TEXT that the kernels include:
//   one row tile per block, 8 waves over the keys (kvz_attn.hip, kvz_retain.hip, kvz_multi.hip)   kvz_decode_state.inc (Q fragment, state),
//                                                       kvz_decode_step.inc (tile step), kvz_decode_loop.inc (key loop), kvz_decode_merge.inc
//   one wave per row tile (kvz_fork_prefill.hip, kvz_multi_prefill.hip)                           kvz_prefill_walk.inc
//   NT row tiles per block (kvz_fork.hip, kvz_spec_step.h for kvz_spec.hip and kvz_tree.hip)      kvz_nt_step.inc, kvz_nt_merge.inc
// A kernel holds what is its own - work-item lookup, addresses and clamped loads, the append, the mask, where partials go - as the
// locals and lambdas a fragment's leading comment asks for.  Text, not functions: as calls into shared function templates each step -
// even the V staging alone, even with the lane handed in - moved the compiler's schedule of the key loop of the decode kernel, while
// included text leaves the device code of every kernel as it was (tools/device_code_diff.py).  A new kernel on this tile includes
// the fragments; a fix to a step is made once.  The combine of the partials, a launch of its own, is shared as a function: kvz_combine.h.
#pragma once
#include "kvz_common.h"

namespace kvz {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));   // (v4, u32x2: the 8-byte output stores of the two prefill kernels)
typedef __bf16 b4 __attribute__((ext_vector_type(4)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef short s8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename T> struct Half;
template <> struct Half<_Float16> {
    typedef h8 v8;
    typedef h4 v4;
    __device__ static inline f4 mfma(v8 a, v8 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct Half<__bf16> {
    typedef b8 v8;
    typedef b4 v4;
    __device__ static inline f4 mfma(v8 a, v8 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

constexpr int TILE_KT = 32;          // keys per wave tile
constexpr int TILE_RT = 16;          // query rows per row tile (MFMA N)

template <int D> struct TileCfg {
    static constexpr int KT = TILE_KT;
    static constexpr int RT = TILE_RT;
    static constexpr int ROW_BYTES = D * 2;
    static constexpr int VSTRIDE = ROW_BYTES + 32;          // padded LDS row: conflict-free tr reads
    static constexpr int WAVE_LDS = KT * VSTRIDE;           // bytes of V staging per wave
    static constexpr int KK = D / 32;                       // MFMA k-steps over the head dim
    static constexpr int DB = D / 16;                       // 16-wide output column blocks
    static constexpr int CPR = ROW_BYTES / 16;              // 16-byte chunks per row
    static constexpr int VLOADS = KT * CPR / WAVE;          // 16-byte V loads per lane per tile
};

constexpr float LOG2E = 1.44269504088896340736f;

// ---- the cut into work items (host; chunk_of also on the device) ---------------------------------------------------------------------

// keys per work item: `total` keys cut into about `target` key ranges, a multiple of 128 keys (4 tiles) and at least 128
template <typename I>
__host__ __device__ static inline I chunk_of(I total, int target) {
    I chunk = (total + target - 1) / target;
    chunk = (chunk + 127) / 128 * 128;
    return chunk < 128 ? 128 : chunk;
}

// Work items a call over `segments` ragged segments is cut into.  Default (knob 0): CUs - segments (256 - Hkv for one cache on MI355X),
// the most that can never exceed one block per CU (every segment rounds its item count up, so a call has at most target + segments
// items; one item beyond 256 costs a second round of blocks: 25 -> 34 us per layer, profiles/r4_decode_cold_probe.txt).  Round 2 had
// settled on 192 with a probe whose single 80-MB cache lived in the infinity cache; streaming a whole model's caches from cold HBM,
// 252 items are 3 % faster than 192.
static inline int target_items(int segments) {
    const int t = tunable(TUNE_ATTN_ITEMS);
    if (t > 0) return t;
    const int cus = device_cus();
    return segments < cus * 3 / 4 ? cus - segments : cus / 4;
}

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// CALL(T, D) for the element type and head dim of a call ({f16, bf16} x {64, 128}, checked by the caller); CALL is a macro of the
// call site and usually returns
#define KVZ_DISPATCH_HALF_D(dtype, D, CALL)                   \
    do {                                                      \
        if ((dtype) == KVZ_F16) {                             \
            if ((D) == 128) { CALL(_Float16, 128); }          \
            else { CALL(_Float16, 64); }                      \
        } else {                                              \
            if ((D) == 128) { CALL(__bf16, 128); }            \
            else { CALL(__bf16, 64); }                        \
        }                                                     \
    } while (0)

}  // namespace kvz
