// mfma_fold_tile_body.hpp -- NOT a header: one wave's tile of multifold_mfma_kernel (mfma_fold.hpp, which describes it), as text: from
// the first loads to the 17 unreduced limbs x[] of this lane's output.  Included inside that kernel alone (the fold workgroups of
// fold_rounds_kernel, fold_rounds.hpp, loop over tiles and have the same steps as code of their own).  It reads, and expects in scope where it is included, exactly: the constants WAVES and DEPTH;
// the kernel arguments in, m, weights, rot; the LDS pointers and arrays qd, q_lds, d_lds, kc_lds, kv_lds; tid, n, h, n_terms; tile.
// It declares row, p, chunk, plane, qa, start, last, term_in_chunk, term_of, da, db, acc00 .. acc11, x and carry, and contains the
// workgroup's barriers: every wave of the workgroup must pass through it.  Text and not a __device__ function for the reason given in sumcheck_small_body.hpp:
// behind a shared function multifold_mfma_kernel<4, 4> came out with another register allocation, and the proofs in flight read 1 % slower.
    const size_t row = 32 * m;                                       // bytes between consecutive terms of one output
    const unsigned char* p = reinterpret_cast<const unsigned char*>(in) + 32 * (tile * 64 + n) + 16 * h;
    const uint32_t chunk = n_terms < (uint32_t)MFM_CHUNK ? n_terms : (uint32_t)MFM_CHUNK;   // terms per chunk, a power of two
    const uint32_t plane = mfm_plane_dwords(chunk);
    // this lane's window of a term's string starts at byte s = 31 - n + 16 h (columns 32..63, mh = 1) and s + 32 (columns 0..31):
    // plane s % 4, dword s / 4 (+ 8 for mh = 0)
    const uint32_t* qa = qd + ((31 - n + 16 * h) & 3) * plane + ((31 - n + 16 * h) >> 2);
    const uint32_t start = (uint32_t)(tile * rot) & (chunk - 1);     // this tile's first term inside every chunk
    const uint32_t last = n_terms - 1;
    // step s of the wave's stream: chunk s / chunk, term ((s % chunk) + start) % chunk of it; steps past the end are clamped
    // to the last one and never used
    // u-th term this tile takes inside a chunk.  (Measured and dropped: the upper half of the table -- what the sums pass read
    // last and the Infinity Cache may still hold -- first, rotated inside each half: 104 us against 93-96 on the same box.)
    auto term_in_chunk = [&](uint32_t u) -> uint32_t { return (u + start) & (chunk - 1); };
    auto term_of = [&](uint32_t s) -> uint32_t {
        s = s < last ? s : last;
        return (s & ~(chunk - 1)) | term_in_chunk(s & (chunk - 1));
    };
    mf_v4i da[DEPTH][2], db[DEPTH][2];
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) { const unsigned char* pt = p + (size_t)term_of(u) * row; da[u][0] = mfm_load_nt(pt); da[u][1] = mfm_load_nt(pt + 1024); }
    if (tid < 64) kc_lds[tid] = 0;
    mf_v16i acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};    // acc[jh][mh]

    for (uint32_t t0 = 0; t0 < n_terms; t0 += chunk) {
        __syncthreads();                                             // the previous chunk's strings are no longer read
        for (uint32_t idx = tid; idx < 4 * chunk; idx += 64 * WAVES) {
            // signed digits: S = W + 0x80...80 (no overflow: W < r < 0.46 * 2^256), digit bytes = S ^ 0x80...80
            const uint32_t t = idx >> 2, a = idx & 3;
            const Fr w = load_fr(weights, t0 + t);
            uint32_t qs[25];                                         // the string as dwords: 8 zero, 8 of digits (reversed), 8 zero, and one more
            uint64_t c = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) { qs[i] = 0; qs[16 + i] = 0; }
            qs[24] = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) { c += (uint64_t)w.l[i] + 0x80808080u; qs[15 - i] = __builtin_bswap32((uint32_t)c ^ 0x80808080u); c >>= 32; }
            uint32_t* q = qd + a * plane + t * 24;
#pragma unroll
            for (int d = 0; d < 24; ++d) q[d] = (uint32_t)((((uint64_t)qs[d + 1] << 32) | qs[d]) >> (8 * a));
        }
        __syncthreads();
        if (tid < 32) {                                              // digit x of every term of the chunk: Q[t][63 - x]
            int32_t dsum = 0;
            for (uint32_t t = 0; t < chunk; ++t) dsum += (int32_t)(signed char)q_lds[t * MFM_QSTRIDE + 63 - tid];
            d_lds[tid] = dsum;
        }
        __syncthreads();
        if (tid < 64) {                                              // column c collects digits c - 31 .. c
            int32_t s = 0;
            const int lo = (int)tid - 31 < 0 ? 0 : (int)tid - 31, hi = tid < 31 ? (int)tid : 31;
            for (int x = lo; x <= hi; ++x) s += d_lds[x];
            kc_lds[tid] += 128 * s;
        }
        // ---- the chunk's terms, DEPTH at a time, two register sets
        for (uint32_t t = 0; t < chunk; t += 2 * DEPTH) {
            const uint32_t g = t0 + t;                                   // step index of da[0]
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) { const unsigned char* pt = p + (size_t)term_of(g + DEPTH + u) * row; db[u][0] = mfm_load_nt(pt); db[u][1] = mfm_load_nt(pt + 1024); }
            __builtin_amdgcn_sched_barrier(0);                       // keep the issue order: the scheduler sank these loads below the MFMAs they should overlap
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) {
                const uint32_t* qt = qa + term_in_chunk(t + u) * 24;
                const mf_v4i a0 = {(int)qt[8], (int)qt[9], (int)qt[10], (int)qt[11]}, a1 = {(int)qt[0], (int)qt[1], (int)qt[2], (int)qt[3]};
                const mf_v4i b0 = mfm_signed(da[u][0]), b1 = mfm_signed(da[u][1]);
                acc00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc00, 0, 0, 0);
                acc01 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc01, 0, 0, 0);
                acc10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc10, 0, 0, 0);
                acc11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc11, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) { const unsigned char* pt = p + (size_t)term_of(g + 2 * DEPTH + u) * row; da[u][0] = mfm_load_nt(pt); da[u][1] = mfm_load_nt(pt + 1024); }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) {
                const uint32_t* qt = qa + term_in_chunk(t + DEPTH + u) * 24;
                const mf_v4i a0 = {(int)qt[8], (int)qt[9], (int)qt[10], (int)qt[11]}, a1 = {(int)qt[0], (int)qt[1], (int)qt[2], (int)qt[3]};
                const mf_v4i b0 = mfm_signed(db[u][0]), b1 = mfm_signed(db[u][1]);
                acc00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc00, 0, 0, 0);
                acc01 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc01, 0, 0, 0);
                acc10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc10, 0, 0, 0);
                acc11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc11, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();
    if (tid < 16) {
        long long v = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) v += (long long)kc_lds[4 * tid + t] << (8 * t);
        kv_lds[tid] = v;
    }
    __syncthreads();
    // ---- epilogue: lane (n, h) takes output 32 h + n.  Result register r = 4 q + t of acc[jh][mh] holds column
    // 32 mh + 8 q + 4 h + t of output 32 jh + n; the swap hands the upper lanes' jh = 0 rows to the lower lanes and the lower
    // lanes' jh = 1 rows to the upper ones: afterwards acc0* holds the h' = 0 rows and acc1* the h' = 1 rows of MY output
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        auto s0 = __builtin_amdgcn_permlane32_swap((unsigned)acc00[r], (unsigned)acc10[r], false, false);
        acc00[r] = (int)s0[0]; acc10[r] = (int)s0[1];
        auto s1 = __builtin_amdgcn_permlane32_swap((unsigned)acc01[r], (unsigned)acc11[r], false, false);
        acc01[r] = (int)s1[0]; acc11[r] = (int)s1[1];
    }
    uint32_t x[18];
    long long carry = 0;
#pragma unroll
    for (int g = 0; g < 16; ++g) {                                   // limb g = columns 4 g .. 4 g + 3 = (mh, q, h') = (g / 8, (g / 2) % 4, g % 2)
        const int mh = g >> 3, q = (g >> 1) & 3, hp = g & 1;
        long long v = carry + kv_lds[g];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int r = 4 * q + t;
            const int col = hp ? (mh ? acc11[r] : acc10[r]) : (mh ? acc01[r] : acc00[r]);
            v += (long long)col << (8 * t);
        }
        x[g] = (uint32_t)v;
        carry = v >> 32;
    }
    x[16] = (uint32_t)carry;
    x[17] = 0;
