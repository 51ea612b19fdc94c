// kvz_decode_merge.inc — the end of a family D kernel: the merge of the block's waves through LDS (each wave writes only its own
// region) and the store of the item's partial (m, l, a[D] per query row).  Text rather than a function: DESIGN.md 3.12.
// Expects in scope:  what kvz_decode_state.inc defines, lds, wl, BLOCK_WAVES (constexpr), part_o, part_ml, and
//                    pbase (int64_t): the first partial row of this (item, row tile).
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    // Rows of D + 4 floats: with a stride of D floats (512 B) the 16 lanes of a quad - 16 query rows, the same output columns -
    // all hit one LDS bank (round 5: 16-way conflict on every store, ~1 us per block, found by ablation: profiles/r5_decode_ablation.txt);
    // the padded row puts the 16-byte stores of 8 consecutive query rows on 8 different bank groups.  Only valid query rows are
    // written and merged (decode: G of the 16).  The NT-row-tile kernels (kvz_fork.hip, kvz_spec_step.h) stage the same way.
    constexpr int WSTR = D + 4;                          // floats per staged row
    static_assert((TILE_RT * WSTR + 2 * TILE_RT) * 4 <= C::WAVE_LDS, "the wave's V tile holds its merge staging");
    float* wo = reinterpret_cast<float*>(wl);            // [16 q][D + 4]
    float* wm = wo + TILE_RT * WSTR;                       // [16] m, [16] l
    const int rows_valid = min(TILE_RT, n_qrows - rt * TILE_RT);
    if (l15 < rows_valid) {
#pragma unroll
        for (int db = 0; db < C::DB; ++db) *reinterpret_cast<f4*>(wo + l15 * WSTR + db * 16 + quad * 4) = o[db];
        if (quad == 0) { wm[l15] = m_run; wm[16 + l15] = l_run; }
    }
    __syncthreads();

    for (int e = threadIdx.x; e < rows_valid * (D / 4); e += BLOCK_WAVES * WAVE) {
        const int qq = e / (D / 4), d = (e % (D / 4)) * 4;
        float mw[BLOCK_WAVES], M = -INFINITY;
#pragma unroll
        for (int w = 0; w < BLOCK_WAVES; ++w) {
            mw[w] = reinterpret_cast<const float*>(lds + w * C::WAVE_LDS)[TILE_RT * WSTR + qq];
            M = fmaxf(M, mw[w]);
        }
        f4 acc4 = f4{0.f, 0.f, 0.f, 0.f};
        float lsum = 0.f;
#pragma unroll
        for (int w = 0; w < BLOCK_WAVES; ++w) {
            const float* pw = reinterpret_cast<const float*>(lds + w * C::WAVE_LDS);
            const float wgt = (mw[w] == -INFINITY) ? 0.f : exp2f(mw[w] - M);
            const f4 ov = *reinterpret_cast<const f4*>(pw + qq * WSTR + d);
            acc4[0] += wgt * ov[0]; acc4[1] += wgt * ov[1]; acc4[2] += wgt * ov[2]; acc4[3] += wgt * ov[3];
            lsum += wgt * pw[TILE_RT * WSTR + 16 + qq];
        }
        *reinterpret_cast<f4*>(part_o + (pbase + qq) * D + d) = acc4;
        if (d == 0) *reinterpret_cast<float2*>(part_ml + (pbase + qq) * 2) = make_float2(M, lsum);
    }
