// kvz_prefill_walk.inc — the walk of ONE wave over the keys of its row tile in the two packed-prefill kernels (family P:
// fork_prefill_kernel, multi_prefill_split_kernel): Q fragment, softmax state, the tile step (V staging, S^T = K.Q^T, online softmax,
// O^T += V^T.P^T), the key loop with the next tile requested - unconditionally: clamped rows - before the current one is computed, and
// the rotation of the two register buffers.  No wave shares anything with another one: no barrier.  Text rather than a function:
// DESIGN.md 3.12.
// Expects in scope:  T, D, C = TileCfg<D>, v8, lane, l15, quad, wl (the wave's LDS tile), scale,
//                    q, qs_head, qs_group, qs_pos, h, cu0, and of this lane's query row: rvalid, p_l, g_l, limit (it sees key < limit);
//                    k0, kend: the keys the wave visits (kend > k0);
//                    load_k(kr, t0), load_v(vr, t0): the kernel's loads of the K fragments and V rows of the tile at key t0, rows
//                    past kend - 1 clamped to it.
// Defines:           sl2, qf[], m_run, l_run, o[] (the state after the last tile), kraw, vraw, knext, vnext, compute_tile.
    const float sl2 = scale * LOG2E;      // work in the exp2 domain

    // stationary Q fragment (B operand of S^T = K.Q^T): col = query row, k = head-dim slice
    v8 qf[C::KK];
    {
        const T* qp = q + (rvalid ? h * qs_head + g_l * qs_group + (int64_t)(cu0 + p_l) * qs_pos : 0) + quad * 8;
#pragma unroll
        for (int kk = 0; kk < C::KK; ++kk) {
            u32x4 raw = *reinterpret_cast<const u32x4*>(qp + kk * 32);
            if (!rvalid) raw = u32x4{0, 0, 0, 0};
            qf[kk] = __builtin_bit_cast(v8, raw);
        }
    }
    float m_run = -INFINITY, l_run = 0.f;
    f4 o[C::DB];
#pragma unroll
    for (int db = 0; db < C::DB; ++db) o[db] = f4{0.f, 0.f, 0.f, 0.f};

    auto compute_tile = [&](u32x4 (&kr)[2][C::KK], u32x4 (&vr)[C::VLOADS], int t0) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < C::VLOADS; ++it) {
            const int c = it * WAVE + lane;
            *reinterpret_cast<u32x4*>(wl + (c / C::CPR) * C::VSTRIDE + (c % C::CPR) * 16) = vr[it];
        }
        f4 sc[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            sc[sub] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < C::KK; ++kk) sc[sub] = Half<T>::mfma(__builtin_bit_cast(v8, kr[sub][kk]), qf[kk], sc[sub]);
        }
        float sv[8];
        float tmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int key = t0 + (j >> 2) * 16 + quad * 4 + (j & 3);
            float x = sc[j >> 2][j & 3] * sl2;
            x = key < limit ? x : -INFINITY;                // the causal diagonal of THIS row, and the end of the keys
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
        for (int db = 0; db < C::DB; ++db) {
            o[db][0] *= alpha; o[db][1] *= alpha; o[db][2] *= alpha; o[db][3] *= alpha;
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

    // the wave's key tiles, the next one requested (unconditionally: clamped rows) before the current one is computed
    u32x4 kraw[2][C::KK], vraw[C::VLOADS], knext[2][C::KK], vnext[C::VLOADS];
    load_k(kraw, k0);
    load_v(vraw, k0);
#pragma unroll 1
    for (int t0 = k0; t0 < kend; t0 += TILE_KT) {
        load_k(knext, t0 + TILE_KT);
        load_v(vnext, t0 + TILE_KT);
        compute_tile(kraw, vraw, t0);
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int kk = 0; kk < C::KK; ++kk) kraw[sub][kk] = knext[sub][kk];
#pragma unroll
        for (int it = 0; it < C::VLOADS; ++it) vraw[it] = vnext[it];
    }
