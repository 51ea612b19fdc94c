// kvz_nt_merge.inc — the end of a family N block (fork_attn_kernel, spec_item): the merge of the block's waves through LDS, one row
// tile after the other (each wave stages in its own V tile), and the store of the partials (m, l, a[D] per query row).  Text rather
// than a function: DESIGN.md 3.12.
// Expects in scope:  T, D, NT, C = TileCfg<D>, l15, quad, lds, wl, BLOCK_WAVES (constexpr), m_run[NT], l_run[NT], o[NT][],
//                    rows_valid[NT], po, pml (where the partials go), slot0 (int64_t) and rt_first: row tile i of the block writes
//                    its valid rows from partial row slot0 + (rt_first + i) * 16 on.
    // ---- merge the 8 waves of the block through LDS, one row tile after the other (each wave stages in its own V tile) ----
    constexpr int WSTR = D + 4;                          // floats per staged row (bank-conflict-free: kvz_decode_merge.inc)
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
        const int64_t pbase = slot0 + (int64_t)(rt_first + i) * TILE_RT;
        for (int e = threadIdx.x; e < rv * (D / 4); e += BLOCK_WAVES * WAVE) {
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
            *reinterpret_cast<f4*>(po + (pbase + qq) * D + d) = acc4;
            if (d == 0) *reinterpret_cast<float2*>(pml + (pbase + qq) * 2) = make_float2(M, lsum);
        }
        __syncthreads();  // (the staging of this row tile has been read: the next one - or the next V tiles - may overwrite it)
    }
