// kvz_decode_step.inc — the tile step of family D (one row tile per block, 8 waves striding over the keys): one 32-key tile of this
// wave, S^T = K.Q^T, online softmax, V through the wave's LDS tile, O^T += V^T.P^T.  Text rather than a function: DESIGN.md 3.12.
// Expects in scope:  what kvz_decode_state.inc defines, lane, wl (the wave's LDS tile), scale, and
//                    visible(key) -> bool: the mask of this lane's query row, a lambda of the kernel.
// Defines:           sl2, kraw, vraw, knext, vnext (the registers of the current and the next tile) and compute_tile(kr, vr, t0).
    const float sl2 = scale * LOG2E;  // work in the exp2 domain
    u32x4 kraw[2][C::KK], vraw[C::VLOADS], knext[2][C::KK], vnext[C::VLOADS];
    auto compute_tile = [&](const u32x4 (&kr)[2][C::KK], const u32x4 (&vr)[C::VLOADS], int t0) __attribute__((always_inline)) {
        f4 sc[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            sc[sub] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < C::KK; ++kk)
                sc[sub] = Half<T>::mfma(__builtin_bit_cast(v8, kr[sub][kk]), qf[kk], sc[sub]);
        }
#pragma unroll
        for (int it = 0; it < C::VLOADS; ++it) {
            const int c = it * WAVE + lane;
            *reinterpret_cast<u32x4*>(wl + (c / C::CPR) * C::VSTRIDE + (c % C::CPR) * 16) = vr[it];
        }
        float sv[8];
        float tmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int key = t0 + (j >> 2) * 16 + quad * 4 + (j & 3);
            float x = sc[j >> 2][j & 3] * sl2;
            x = visible(key) ? x : -INFINITY;
            sv[j] = x;
            tmax = fmaxf(tmax, x);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float m_new = fmaxf(m_run, tmax);
        const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;
        const float alpha = exp2f(m_run - m_safe);
        float psum = 0.f;
        v8 pb;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float p = exp2f(sv[j] - m_safe);
            psum += p;
            pb[j] = (T)p;
        }
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int i = 0; i < C::DB; ++i) {
            o[i][0] *= alpha; o[i][1] *= alpha; o[i][2] *= alpha; o[i][3] *= alpha;
        }
        const char* trp = wl + (quad * 4 + (l15 >> 2)) * C::VSTRIDE + (l15 & 3) * 8;
#pragma unroll
        for (int db = 0; db < C::DB; ++db) {
            s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(trp + db * 32));
            s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(trp + 16 * C::VSTRIDE + db * 32));
            s8 both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            o[db] = Half<T>::mfma(__builtin_bit_cast(v8, both), pb, o[db]);
        }
    };
