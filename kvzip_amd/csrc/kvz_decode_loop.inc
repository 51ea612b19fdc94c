// kvz_decode_loop.inc — the key loop of family D where a tile's rows are addressed by the key alone (varlen_attn_split2_kernel,
// multi_attn_split_kernel; retain_attn_kernel keeps a loop of its own, which also looks ahead in its index).  Text rather than a
// function: DESIGN.md 3.12.
// Expects in scope:  what kvz_decode_step.inc defines, wave, c0, c1 (the key range of the item), BLOCK_WAVES (constexpr), and
//                    load_tile(kr, vr, t0): the kernel's clamped loads of the K fragments and V rows of the tile at key t0.
//
// The wave's tiles, one requested AHEAD of the one being computed.  Round 4: the steady-state loop issues the next tile's loads
// UNCONDITIONALLY and the last tile is computed after the loop.  With the request inside `if (tn < c1)` the compiler has to place
// waits that are right on both paths - s_waitcnt vmcnt(7) .. vmcnt(0) before the V rows of the CURRENT tile go to LDS - which
// drains the tile that has just been requested in the middle of every iteration: no load was ever in flight while a wave
// computed, and the kernel ran at 21 us where the bare read stream takes 12.5 (profiles/r4_probe_stream.txt).
    const int t_first = c0 + wave * TILE_KT;
    constexpr int T_STEP = BLOCK_WAVES * TILE_KT;
    if (t_first < c1) {
        load_tile(kraw, vraw, t_first);
        int t0 = t_first;
#pragma unroll 1
        for (; t0 + T_STEP < c1; t0 += T_STEP) {
            load_tile(knext, vnext, t0 + T_STEP);
            compute_tile(kraw, vraw, t0);
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int kk = 0; kk < C::KK; ++kk) kraw[sub][kk] = knext[sub][kk];
#pragma unroll
            for (int it = 0; it < C::VLOADS; ++it) vraw[it] = vnext[it];
        }
        compute_tile(kraw, vraw, t0);
    }
