// kvz_nt_step.inc — the tile step and the key loop of the kernels whose blocks own NT row tiles (family N: fork_attn_kernel in
// kvz_fork.hip and spec_item in kvz_spec_step.h, which serves spec_attn_kernel and tree_attn_kernel).  Text rather than a function:
// DESIGN.md 3.12.
// Expects in scope:  T, D, NT, C = TileCfg<D>, v8, lane, wave, l15, quad, wl (the wave's LDS tile), sl2, BLOCK_WAVES (constexpr),
//                    c0, c1 (the key range of the item),
//                    qf[NT][], m_run[NT], l_run[NT], o[NT][] (Q fragments and softmax state per row tile),
//                    load_k(kr, t0), load_v(vr, t0): the kernel's clamped loads of the K fragments and V rows of the tile at key t0,
//                    KVZ_NT_VISIBLE(i, key): the mask of this lane's query row of row tile i, an expression.  A MACRO, undefined
//                    again below: as a lambda of the kernel (always_inline or not) it changed the device code of all 8
//                    fork_attn_kernel instantiations and of tree_attn_kernel at NT = 1.
// Defines:           VLATE, kraw, vraw, knext, vnext, compute_tile(kr, vr, t0, t_next, refill) - refill = std::true_type requests
//                    the rows of the tile at t_next into kr / vr as soon as the step has spent them - and runs the key loop.
    // Two row tiles at head dim 128 leave no registers for a second K and V buffer (with them 51 registers spilled to scratch): there
    // the next tile's V rows are requested into the SAME registers right after the current ones have gone to LDS, and its K rows
    // right after the S^T products have consumed the current ones - still unconditionally, and in flight during the softmax and
    // the P.V products of the current tile.
    constexpr bool VLATE = NT * D > 128;
    u32x4 kraw[2][C::KK], vraw[C::VLOADS], knext[VLATE ? 1 : 2][C::KK], vnext[VLATE ? 1 : C::VLOADS];
    // one 32-key tile of this wave, applied to the NT row tiles: the K fragments feed NT S^T = K.Q^T products, the V tile goes
    // through the wave's LDS tile once and every transposed fragment read back from it feeds NT O^T += V^T.P^T products
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
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = t0 + (j >> 2) * 16 + quad * 4 + (j & 3);
                float x = s[i][j >> 2][j & 3] * sl2;
                x = KVZ_NT_VISIBLE(i, key) ? x : -INFINITY;
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
#undef KVZ_NT_VISIBLE
    // The wave's tiles, one requested AHEAD of the one being computed; the steady-state loop issues the next tile's loads
    // UNCONDITIONALLY and the last tile is computed after the loop (the load structure of kvz_decode_loop.inc: its comment records
    // what the conditional form cost).
    const int t_first = c0 + wave * TILE_KT;
    constexpr int T_STEP = BLOCK_WAVES * TILE_KT;
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
