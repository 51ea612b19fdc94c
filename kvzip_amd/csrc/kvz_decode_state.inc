// kvz_decode_state.inc — the stationary Q fragment and the softmax state of a block that owns ONE row tile of 16 query rows (family D:
// varlen_attn_split2_kernel, retain_attn_kernel, multi_attn_split_kernel).  Text rather than a function: DESIGN.md 3.12.
// Expects in scope:  T, D, C = TileCfg<D>, v8, l15, quad, rt (the block's row tile),
//                    q, q_row0 (int64_t: the first of the query rows this block's head or segment owns in q), n_qrows (how many it owns).
// Defines:           qrow, qvalid, qf[], m_run, l_run, o[].
    // ---- stationary Q fragment (B operand of S^T = K.Q^T): col = query row, k = head-dim slice ----
    const int qrow = rt * TILE_RT + l15;
    const bool qvalid = qrow < n_qrows;
    v8 qf[C::KK];
    {
        const T* qp = q + (q_row0 + (qvalid ? qrow : 0)) * D + quad * 8;
#pragma unroll
        for (int kk = 0; kk < C::KK; ++kk) {
            u32x4 raw = *reinterpret_cast<const u32x4*>(qp + kk * 32);
            if (!qvalid) raw = u32x4{0, 0, 0, 0};
            qf[kk] = __builtin_bit_cast(v8, raw);
        }
    }
    float m_run = -INFINITY, l_run = 0.f;
    f4 o[C::DB];
#pragma unroll
    for (int i = 0; i < C::DB; ++i) o[i] = f4{0.f, 0.f, 0.f, 0.f};
