// kvz_spec_block.inc — the body of a block of the verify step, included by the attention kernel of each form (spec_attn_kernel in
// kvz_spec.hip, tree_attn_kernel in kvz_tree.hip: they differ in the mask of the triangle item alone).  The including kernel has the
// parameters of spec_attn_kernel in scope and defines
//   KVZ_SPEC_TREE   false / true: the mask policy of the triangle item (spec_item's TREE)
//   KVZ_SPEC_ANC    nullptr / the address of the kernel's AncMasks argument
// Text rather than a function: see kvz_spec_step.h.
// Partial rows of the workspace: item i, row tile rt -> (i * n_rtiles + rt) * 16 rows; items 0 .. Hkv - 1 are the triangles of the
// heads, the shared work items follow in head order.
    typedef TileCfg<D> C;
    __shared__ __attribute__((aligned(16))) char lds[SP_WAVES * C::WAVE_LDS];
    const int R = t * G;
    const int rt0 = (int)blockIdx.y * NT;
    if (rt0 >= n_rtiles) return;
    auto len_of = [&](int hh) -> int { return (host_meta ? hm.len[hh] : k_len[hh]) + k_len_offset; };

    if ((int)blockIdx.x < Hkv) {
        // ---- triangle item: the row tiles of this group over the t new keys, read from k_new / v_new ----
        const int h = blockIdx.x;
        const T* kn = k_new + h * kn_hstride;
        const T* vn = v_new + h * vn_hstride;
        if (blockIdx.y == 0) {
            // the t new rows of head h go behind its segment: the only bytes of the cache this launch writes, and nothing reads them
            constexpr int CH = D * 2 / 16;
            const int64_t row0 = (int64_t)(host_meta ? hm.start[h] : k_start[h]) + len_of(h);
            for (int e = threadIdx.x; e < 2 * t * CH; e += SP_THREADS) {
                const bool is_v = e >= t * CH;
                const int i = e - (is_v ? t * CH : 0);
                const int p = i / CH, c = i - p * CH;
                const T* src = (is_v ? vn + p * vn_pstride : kn + p * kn_pstride) + c * 8;
                T* dst = (is_v ? v : k) + (row0 + p) * D + c * 8;
                *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
            }
        }
        // (the last row of the group sees the most keys: later ones are masked for every row of this block)
        const int last_row = min(R, (rt0 + NT) * TILE_RT) - 1;
        const int c1 = last_row / G + 1;
        spec_item<T, D, NT, true, KVZ_SPEC_TREE>(q, reinterpret_cast<const char*>(kn), reinterpret_cast<const char*>(vn), kn_pstride * 2,
                                        vn_pstride * 2, t, 0, c1, h, R, G, rt0, scale, part_o, part_ml,
                                        ((int64_t)h * n_rtiles + rt0) * TILE_RT, lds, KVZ_SPEC_ANC);
        return;
    }

    // ---- shared work item (wave-uniform scalar work) ----
    int total = 0;
    for (int hh = 0; hh < Hkv; ++hh) total += len_of(hh);
    const int chunk = chunk_of(total, target_items);
    int split = 0, first_item = 0, h = -1;
    {
        int bx = (int)blockIdx.x - Hkv, items = 0;
        for (int hh = 0; hh < Hkv; ++hh) {
            const int n = max(1, (len_of(hh) + chunk - 1) / chunk);  // (an empty head still gets one item: it writes zeros)
            if (h < 0) {
                if (bx < n) { h = hh; split = bx; first_item = items; }
                else bx -= n;
            }
            items += n;
        }
    }
    if (h < 0) return;  // beyond the last item
    const int len = len_of(h);
    const int64_t seg = host_meta ? hm.start[h] : k_start[h];
    const int c0 = split * chunk;
    const int c1 = min(len, c0 + chunk);
    spec_item<T, D, NT, false>(q, reinterpret_cast<const char*>(k) + seg * C::ROW_BYTES, reinterpret_cast<const char*>(v) + seg * C::ROW_BYTES,
                               C::ROW_BYTES, C::ROW_BYTES, len, c0, c1, h, R, G, rt0, scale, part_o, part_ml,
                               ((int64_t)(Hkv + first_item + split) * n_rtiles + rt0) * TILE_RT, lds);
